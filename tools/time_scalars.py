"""Timing of the diffusing scalar channels (include/sph_abi.h "diffusing scalar fields") at config 3 (4 M particles, 128^3 cells), on the
lattice state (substep 1) and after 300 substeps (the compressed regime).  For K = 1 and K = 4 and both forms of
the sweep (SPH_OPT_SCALAR_SWEEP 0: global walk, 1: LDS-staged):

  scalar_work   what one substep spends on the scalars (k_scalar_gather + the sweep): the engine's own device events around those two
                launches (SPH_OPT_TIMING, class `other`, one bracket per dispatch), beside class `sph` (the SPH pass) of the same
                dispatches and their ratio
  gather        k_scalar_gather alone: class `other` of a scalar sample call with no probes (its grid build is timed under the
                bin / scan / scatter classes); sweep = scalar_work - gather
  whole_substep device events around sph_dispatch_n(8) with no scalars, K = 1 and K = 4 (shipped sweep form), per substep
  no_scalars    launches per class of 8 dispatches on an engine that never had scalars, and on one whose scalars were dropped:
                both must be what the engine launched before the feature existed (bin 1, scan 1, scatter 1, sph 1 per dispatch)

and, without a GPU (the host twin on tests/golden/settled_pool.npz, frozen state): the effective-diffusivity factor of DESIGN.md
section 3h, the decay rate of the lowest vertical mode of a painted step profile against (D / rho) k^2.

Device events on the engine's stream, warm-up, median and p10-p90 of the samples (run-to-run spread: p10-p90).
  python tools/time_scalars.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
  python tools/time_scalars.py --factor            (the CPU part alone)
Without an argument the result goes to time_scalars.json in the current directory; profiles/r12_time_scalars.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

import timing
from timing import REPS, ROOT, other_us, pkg, stats

F = np.float32


def effective_factor():
    """Lowest vertical mode on the settled pool, frozen state, host twin: a step painted at mid height, projected on cos(pi (y - y0) / H)."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "settled_pool.npz"))
    rec, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    fluid = rec["isGhost"] == 0
    y = rec["pos"][:, 1].astype(np.float64)
    y0, y1 = y[fluid].min(), y[fluid].max()
    H = y1 - y0
    k = np.pi / H
    mode = np.cos(k * (y - y0))
    mode = mode - mode[fluid].mean()                                     # (the conserved mean of the field projects on nothing)
    c = (y > 0.5 * (y0 + y1)).astype(F)
    _, s1 = pkg.scalars_step_host(rec, sp, c, diffusivity=1.0)
    D = F(0.5 / float(s1))
    rho = float(rec["density"][fluid].astype(np.float64).mean())
    amp = [float((c.astype(np.float64) * mode)[fluid].sum())]
    steps = 80
    for _ in range(steps):
        c, s = pkg.scalars_step_host(rec, sp, c, diffusivity=D)
        c = c[:, 0]
        amp.append(float((c.astype(np.float64) * mode)[fluid].sum()))
    dt = float(F(sp.param_timeStep))
    nominal = float(D) / rho * k * k
    factor = lambda a, b: (1.0 - (amp[b] / amp[a]) ** (1.0 / (b - a))) / dt / nominal
    return {"state": "tests/golden/settled_pool.npz (frozen)", "particles": int(len(rec)), "mean_density": rho, "depth_over_h": float(H / float(F(sp.param_h))),
            "diffusion_number": float(s), "substeps": steps, "nominal_rate_per_s": float(nominal),
            "factor_substeps_0_40": float(factor(0, 40)), "factor_substeps_40_80": float(factor(40, 80))}


def coefficients(K, state, sp):
    """Diffusivities for a diffusion number of about 0.4 (from one engine substep with D = 1), channel k at D / (k + 1)."""
    e = pkg.SPHFluidGPU.from_particles(state, sp)
    e.set_scalars(np.zeros(len(state), F), diffusivity=1.0)
    e.DispatchCompute()
    s1 = float(e.scalar_info()[1])
    e.close()
    return (F(0.4 / s1) / np.arange(1, K + 1, dtype=F)).astype(F)


def scalar_work(f, values, D, staged):
    f.set_option(pkg.SPH_OPT_SCALAR_SWEEP, staged)
    f.set_scalars(values, diffusivity=D)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(3):
        f.DispatchCompute()
    f.kernel_times(reset=True)
    work, walk = [], []
    for _ in range(REPS):
        f.DispatchCompute()
        t = f.kernel_times(reset=True)
        assert t["other"][1] == 1, t
        work.append(t["other"][0] * 1000.0)
        walk.append(t["sph"][0] * 1000.0)
    gather = []
    for k in range(3 + REPS):
        f.sample_scalar_device(0, 0, 0)
        us, launches = other_us(f)
        assert launches == 1, launches
        if k >= 3:
            gather.append(us)
    number = float(f.scalar_info()[1])
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    r = {"scalar_work": stats(work), "sph_pass": stats(walk), "gather": stats(gather), "diffusion_number": number}
    r["sweep_us"] = r["scalar_work"]["median_us"] - r["gather"]["median_us"]
    r["scalar_work_over_sph_pass"] = r["scalar_work"]["median_us"] / r["sph_pass"]["median_us"]
    return r


def launch_counts(f, n=8):
    f.DispatchCompute()                                                  # (the first dispatch after an upload also imports the records)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    f.kernel_times(reset=True)
    for _ in range(n):
        f.DispatchCompute()
    t = f.kernel_times(reset=True)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    return {k: int(v[1]) for k, v in t.items()}


def main() -> None:
    if "--factor" in sys.argv[1:]:
        print(json.dumps(effective_factor(), indent=1))
        return
    import torch
    out_path = timing.out_path(sys.argv[1:], "scalars")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    res = timing.header("tools/time_scalars.py", cfg, rec, variant_library=True, samples_per_case=REPS, regimes={})
    rng = np.random.default_rng(7)
    for label, substep, state in timing.regimes(f):
        r = {}
        for K in (1, 4):
            D = coefficients(K, state, sp)
            values = rng.random((len(state), K)).astype(F)
            for staged in (0, 1):
                e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)       # every case starts from the same state
                r[f"K{K}_{'staged' if staged else 'plain'}"] = scalar_work(e, values, D, staged)
                e.close()
                print(label, K, staged, json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r[f"K{K}_{'staged' if staged else 'plain'}"].items()}),
                      flush=True)
            a, b = r[f"K{K}_plain"]["scalar_work"], r[f"K{K}_staged"]["scalar_work"]
            spread = max(a["p90_us"] - a["p10_us"], b["p90_us"] - b["p10_us"])
            r[f"K{K}_staged_faster_by_more_than_the_spread"] = bool(a["median_us"] - b["median_us"] > spread)
        # whole substeps: device events around sph_dispatch_n(8)
        sub = {}
        for name, K in (("no_scalars", 0), ("K1", 1), ("K4", 4)):
            e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
            if K:
                e.set_scalars(rng.random((len(state), K)).astype(F), diffusivity=coefficients(K, state, sp))
            st = timing.events(lambda: e.DispatchN(8), stream, reps=9, warm=2)
            sub[name] = {k: v / 8.0 / 1000.0 if k.endswith("_us") else v for k, v in st.items()}
            sub[name] = {k.replace("_us", "_ms_per_substep"): v for k, v in sub[name].items()}
            e.close()
        r["whole_substep"] = sub
        # the no-scalars path: launches per class of 8 dispatches, never set and set then dropped
        e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
        never = launch_counts(e)
        e.set_scalars(np.zeros(len(state), F), diffusivity=1.0)
        with_scalars = launch_counts(e)
        e.clear_scalars()
        dropped = launch_counts(e)
        e.close()
        r["launches_of_8_dispatches"] = {"never_set": never, "with_scalars": with_scalars, "set_then_dropped": dropped}
        assert never == dropped and never["other"] == 0 and with_scalars["other"] == 8, (never, with_scalars, dropped)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    res["effective_diffusivity"] = effective_factor()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
