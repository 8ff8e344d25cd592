"""Timing of the active scalars (include/sph_abi.h "active scalars") at config 3 (4 M particles, 128^3 cells), on the
lattice state (substep 1) and after 300 substeps (the compressed regime), for K = 1 and K = 4 channels:

  whole_substep   device events around sph_dispatch_n(8), per substep: scalars only, with buoyancy added, and with 8 sources (4 of them
                  riding on bodies; the 4 bodies are present in all three cases, so that the difference is the coupling alone)
  couple_kernels  the coupling kernels' own time: the engine's device events (SPH_OPT_TIMING, class `other`) of single dispatches with
                  the coupling minus those of the same dispatches without it (the class also holds the scalar step and the obstacle
                  step, one bracket each); buoyancy alone (k_scalar_couple<K, false, true>) and 8 sources with buoyancy
                  (k_scalar_couple<K, true, true> + k_scalar_couple_finish)
  copy_yardstick  a plain device-to-device copy that moves the bytes the kernel has to move: pos + vel + K values read, vel + K values
                  written = 48 + 8 K bytes per particle, i.e. a copy of 24 + 4 K bytes per particle, and the ratios against it

Device events on the engine's stream, warm-up, median and p10-p90 of the samples (run-to-run spread: p10-p90).
  python tools/time_coupling.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_coupling.json in the current directory; profiles/r13_time_coupling.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import REPS, pkg, stats
from time_scalars import coefficients

F = np.float32


def scene(state):
    """4 resting bodies and 8 sources (4 in the world frame, 4 riding on the bodies) on a 2 x 2 x 2 grid inside the fluid."""
    centres, r = timing.body_grid(state, 8)
    bodies = [pkg.obstacle(pkg.SPH_OBSTACLE_SPHERE if i % 2 else pkg.SPH_OBSTACLE_BOX, centres[i], r if i % 2 else (r, 0.8 * r, 0.9 * r),
                           rotation=(0.9, 0.1, 0.3, -0.2)) for i in range(4)]
    return bodies, centres, r


def sources_for(K, centres, r):
    src = []
    for i in range(4):
        src.append(pkg.scalar_source(pkg.SPH_SOURCE_SPHERE if i % 2 else pkg.SPH_SOURCE_BOX, (0.0, 0.0, 0.0), 1.6 * r, channel=i % K,
                                     mode=pkg.SPH_SOURCE_RELAX, rate=20.0, target=1.0, body=i))
    for i in range(4, 8):
        src.append(pkg.scalar_source(pkg.SPH_SOURCE_SPHERE if i % 2 else pkg.SPH_SOURCE_BOX, centres[i], 1.2 * r, channel=i % K,
                                     mode=pkg.SPH_SOURCE_RATE if i < 6 else pkg.SPH_SOURCE_RELAX, rate=2.0, target=0.0))
    return src


def other_per_dispatch(e, reps=REPS, warm=3):
    """Class `other` of each of `reps` single dispatches after `warm` warm-ups: the scalar step, the obstacle step and, where it is on,
    the coupling step, one bracket each.  Leaves SPH_OPT_TIMING on."""
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(warm):
        e.DispatchCompute()
    timing.other_us(e)
    us = []
    for _ in range(reps):
        e.DispatchCompute()
        us.append(timing.other_us(e)[0])
    return us


def copy_of(n_floats, stream):
    import torch
    src = torch.ones(n_floats, dtype=torch.float32, device="cuda")
    dst = torch.empty(n_floats, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(stream):
        return timing.events(lambda: dst.copy_(src), stream)


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "coupling")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    res = timing.header("tools/time_coupling.py", cfg, rec, variant_library=True, samples_per_case=REPS, regimes={})
    rng = np.random.default_rng(7)
    n = len(rec)
    for label, substep, state in timing.regimes(f):
        r = {}
        bodies, centres, rad = scene(state)
        for K in (1, 4):
            D = coefficients(K, state, sp)
            values = rng.random((n, K)).astype(F)
            beta, ref = np.full(K, 0.05, F), np.full(K, 0.5, F)
            src = sources_for(K, centres, rad)
            whole, other = {}, {}
            for name in ("scalars_only", "buoyancy", "sources8_buoyancy"):
                e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)           # every case starts from the same state
                e.set_scalars(values, diffusivity=D)
                e.set_obstacles(bodies)
                if name != "scalars_only":
                    e.set_scalar_buoyancy(beta, ref)
                if name == "sources8_buoyancy":
                    e.set_scalar_sources(src)
                other[name] = stats(other_per_dispatch(e))
                e.set_option(pkg.SPH_OPT_TIMING, 0)
                st = timing.events(lambda: e.DispatchN(8), stream, reps=9, warm=2)
                whole[name] = {k.replace("_us", "_ms_per_substep"): (v / 8.0 / 1000.0 if k.endswith("_us") else v) for k, v in st.items()}
                if name == "sources8_buoyancy":
                    sums, hits, _, steps = e.scalar_injected()
                    whole[name]["hits_per_substep"] = [float(h) / max(steps, 1) for h in hits]
                e.close()
            copy = copy_of(n * (6 + K), stream)
            kern = {name: other[name]["median_us"] - other["scalars_only"]["median_us"] for name in ("buoyancy", "sources8_buoyancy")}
            r[f"K{K}"] = {"whole_substep": whole, "class_other_per_dispatch": other, "couple_kernels_us": kern,
                          "copy_yardstick": dict(copy, bytes_per_particle_moved=48 + 8 * K),
                          "couple_over_copy": {name: kern[name] / copy["median_us"] for name in kern}}
            print(label, K, json.dumps({"whole_ms": {k: v["median_ms_per_substep"] for k, v in whole.items()}, "couple_us": kern, "copy_us": copy["median_us"]}), flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
