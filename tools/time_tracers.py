"""Timing of the passive tracers (include/sph_abi.h "passive tracers") at config 3 (4 M particles, 128^3 cells), on the lattice state
(substep 0, after the one substep that gives the records a density) and after 300 substeps (the compressed regime).
For M = 65 536 and 1 048 576 tracers seeded uniformly in the fluid's bounding box, Euler and midpoint:

  tracer_work   what one substep spends on the tracers (k_tracer_advect + k_tracer_tick, and on a substep that re-sorts the processing
                order also the sort): the engine's own device events around those launches (SPH_OPT_TIMING, class `other`), one sample
                per dispatch
  yardstick     k_sample_points on the same positions without its grid build (the same class of the same events around that launch);
                two such calls for the midpoint rule
  refresh       the cell sort of the processing order alone (dispatches whose class `other` holds two brackets, minus the median of
                the others), and that cost divided by the refresh interval

and end to end, wall clock: 100 substeps with 1 M tracers through one sph_dispatch_n call against the host loop over the sampling
interface (sample, host update, dispatch per substep).

Device events on the engine's stream, warm-up, median and p10-p90 of the samples.
  python tools/time_tracers.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_tracers.json in the current directory; profiles/r08_time_tracers.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import os
import re
import sys
import time

import numpy as np

import timing
from timing import ROOT, other_us, pkg, stats

F = np.float32


def refresh_interval() -> int:
    src = open(os.path.join(ROOT, pkg.__name__, "csrc", "sph_tracer.h")).read()
    return int(re.search(r"#define SPH_TRACER_REFRESH\s+(\d+)", src).group(1))


def seeds(state, m, rng):
    fluid = state["pos"][state["isGhost"] == 0][:, :3]
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = (lo + (hi - lo) * rng.random((m, 3))).astype(F)
    return p4


def tracer_work(f, p4, integ, R, reps):
    """Per-dispatch device time of the tracer launches over `reps` consecutive substeps (the state advances: the regime does not)."""
    import torch
    f.set_tracers(p4, integ)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(3):
        f.DispatchCompute()
    other_us(f)
    plain, sorts = [], []
    for _ in range(reps):
        f.DispatchCompute()
        us, launches = other_us(f)
        (sorts if launches > 1 else plain).append(us)
    # the yardstick on the positions the tracers have now
    pos = f.tracers()
    q4 = np.zeros((len(pos), 4), F)
    q4[:, :3] = pos["pos"]
    dev_in = torch.from_numpy(q4).cuda()
    dev_out = torch.empty((len(pos), 8), dtype=torch.float32, device="cuda")
    f.clear_tracers()
    yard = []
    for k in range(3 + max(reps, 25)):
        f.sample_device(dev_in.data_ptr(), len(pos), dev_out.data_ptr())
        us, _ = other_us(f)
        if k >= 3:
            yard.append(us)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    calls = 2 if integ == pkg.SPH_TRACER_MIDPOINT else 1
    r = {"tracer_work": stats(plain), "yardstick_one_call": stats(yard), "yardstick_calls": calls,
         "in_fluid": int((pos["fraction"] >= 0.5).sum())}
    r["yardstick_us"] = calls * r["yardstick_one_call"]["median_us"]
    r["yardstick_over_tracer_work"] = r["yardstick_us"] / r["tracer_work"]["median_us"]
    if sorts:
        extra = float(np.median(sorts)) - r["tracer_work"]["median_us"]
        r["refresh"] = {"dispatches": len(sorts), "extra_us": extra, "interval": R, "amortised_us_per_substep": extra / R}
    return r


def host_loop(f, p4, n, dt, integ):
    x = p4[:, :3].copy()
    for _ in range(n):
        s = f.sample(x)
        v = s["vel"]
        if integ == pkg.SPH_TRACER_MIDPOINT:
            v = f.sample((x + (F(F(0.5) * dt) * v).astype(F)).astype(F))["vel"]
        f.DispatchCompute()
        x = (x + (dt * v).astype(F)).astype(F)
    return x


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "tracers")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    R = refresh_interval()
    reps = 2 * R + 8
    res = timing.header("tools/time_tracers.py", cfg, rec, variant_library=True, refresh_interval=R, samples_per_case=reps, regimes={})
    rng = np.random.default_rng(7)
    for label, substep, state in timing.regimes(f):
        r = {}
        for m in (1 << 16, 1 << 20):
            p4 = seeds(state, m, rng)
            for name, integ in (("euler", pkg.SPH_TRACER_EULER), ("midpoint", pkg.SPH_TRACER_MIDPOINT)):
                e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)        # every case starts from the same state
                r[f"{name}_{m}"] = tracer_work(e, p4, integ, R, reps)
                e.close()
                print(label, name, m, json.dumps({k: (v["median_us"] if isinstance(v, dict) and "median_us" in v else v)
                                                   for k, v in r[f"{name}_{m}"].items()}), flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    # end to end: 100 substeps with 1 M tracers, one sph_dispatch_n call against the host loop over the sampling interface
    p4 = seeds(state, 1 << 20, rng)
    n = 100
    e2e = {}
    for name, integ in (("euler", pkg.SPH_TRACER_EULER), ("midpoint", pkg.SPH_TRACER_MIDPOINT)):
        a = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
        a.set_tracers(p4, integ)
        a.DispatchN(2)
        a.set_tracers(p4, integ)
        a.sync()
        t0 = time.perf_counter()
        a.DispatchN(n)
        a.tracers()                                                      # (synchronises: the caller has its tracers on the host)
        t_engine = time.perf_counter() - t0
        a.close()
        b = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
        host_loop(b, p4, 2, F(sp.param_timeStep), integ)
        b.sync()
        t0 = time.perf_counter()
        host_loop(b, p4, n, F(sp.param_timeStep), integ)
        b.sync()
        t_host = time.perf_counter() - t0
        b.close()
        c = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)      # the substeps alone
        c.DispatchN(2)
        c.sync()
        t0 = time.perf_counter()
        c.DispatchN(n)
        c.sync()
        t_plain = time.perf_counter() - t0
        c.close()
        e2e[name] = {"substeps": n, "tracers": 1 << 20, "dispatch_n_with_tracers_ms": t_engine * 1e3, "host_loop_ms": t_host * 1e3,
                     "dispatch_n_without_tracers_ms": t_plain * 1e3, "host_loop_over_engine": t_host / t_engine}
        print("end_to_end", name, json.dumps(e2e[name]), flush=True)
    res["end_to_end"] = e2e
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
