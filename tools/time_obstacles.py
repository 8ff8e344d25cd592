"""Timing of the obstacle pass (include/sph_abi.h "obstacles") at config 3 (4 M particles, 128^3 cells), on the
lattice state (after the one substep that gives the records a density) and after 300 substeps (the compressed regime).
For K = 1, 4 and 16 spinning, slowly moving bodies (spheres, boxes and capsules in turn) laid out on a grid inside the fluid's bounding box:

  obstacle_pass   what one substep spends on the obstacles (k_obstacles + k_obstacles_finish): the engine's own device events around
                  those two launches (SPH_OPT_TIMING, class `other`; config 3's box container adds nothing else to that class), one sample
                  per dispatch
  yardstick       a device-to-device copy of arrays of the size of the engine's pos + vel state (two float4 per particle), two copies
                  timed with device events on the engine's stream in the same process
  ratio           obstacle_pass / yardstick; the goal is <= 1.25 for K = 1 and K = 4 (K = 16 is reported, not gated)

touched_fraction is the share of records whose position differs after one substep with the bodies from one without them.
  python tools/time_obstacles.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_obstacles.json in the current directory; profiles/r09_time_obstacles.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import REPS, pkg, stats


def bodies(state, K, dt):
    centres, r = timing.body_grid(state, K)
    out = []
    for k, c in enumerate(centres):
        shape = k % 3
        size = (r,) if shape == 0 else ((r, 0.8 * r, 0.6 * r) if shape == 1 else (0.6 * r, 0.7 * r))
        out.append(pkg.obstacle(shape, c, size, rotation=(0.9, 0.1, 0.3, 0.2), vel=(0.02 * r / dt, 0.0, 0.0), omega=(0.0, 0.5 / (16 * dt), 0.1 / (16 * dt))))
    return out


def obstacle_pass(state, sp, stream, K):
    f = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    f.set_obstacles(bodies(state, K, float(sp.param_timeStep)))
    us = timing.other_per_dispatch(f)                                    # one bracket: the two obstacle launches, nothing else
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    J, t, n = f.obstacle_impulses()
    f.close()
    return stats(us), {"substeps": n, "bodies_with_impulse": int((np.abs(J).sum(axis=1) > 0).sum())}


def touched_fraction(state, sp, stream, K):
    a = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    a.set_obstacles(bodies(state, K, float(sp.param_timeStep)))
    return timing.moved_fraction(state, sp, stream, a)


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "obstacles")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    res = timing.header("tools/time_obstacles.py", cfg, rec, variant_library=True, samples_per_case=REPS, regimes={})
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    for label, substep, state in timing.regimes(f, single_step_compute=True):
        yard = timing.copy_yardstick(len(state), stream)
        r = {"substep": substep, "yardstick": yard}
        for K in (1, 4, 16):
            s, info = obstacle_pass(state, sp, stream, K)
            r[f"K{K}"] = {"obstacle_pass": s, "ratio": s["median_us"] / yard["median_us"], "touched_fraction": touched_fraction(state, sp, stream, K), **info}
            print(label, K, json.dumps({"pass_us": s["median_us"], "copy_us": yard["median_us"], "ratio": r[f"K{K}"]["ratio"],
                                        "touched": r[f"K{K}"]["touched_fraction"]}), flush=True)
        res["regimes"][label] = r
    f.close()
    res["goal"] = "K = 1 and K = 4: obstacle_pass <= 1.25 x yardstick"
    res["goal_met"] = all(res["regimes"][g][f"K{K}"]["ratio"] <= 1.25 for g in res["regimes"] for K in (1, 4))
    timing.write_json(res, out_path, "goal met" if res["goal_met"] else "goal NOT met")


if __name__ == "__main__":
    main()
