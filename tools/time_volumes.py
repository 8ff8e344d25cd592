"""Timing of volume-bound obstacles and of the mesh -> signed distance build (include/sph_abi.h "signed distance lattices", DESIGN.md
section 3f), protocol of tools/time_obstacles.py: config 3 (4 M particles, 128^3 cells), on the lattice state and after 300 substeps,
device events (SPH_OPT_TIMING, class `other`), 25 substeps after 3 warm-ups, median [p10, p90].

For K = 1 and K = 4 spinning, slowly moving boxes laid out on a grid inside the fluid's bounding box:
  box_pass      the obstacle pass with plain boxes (k_obstacles: the code path without volumes)
  volume_pass   the same boxes, each bound to the lattice of a sphere that fills the box (k_obstacles_vol)
  yardstick     a device-to-device copy of arrays of the size of pos + vel, timed in the same process
  inside_box    share of the records a plain box moves (every record inside a box: what pays the gathers)
  inside_solid  share of the records the volume-bound body moves
No ratio is gated.

sph_mesh_distance on an icosphere: 128^3 points x 20 480 triangles and 64^3 x 1 280: wall time of the call up to the end of the stream,
device time of its two kernels, pairs per second.
  python tools/time_volumes.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_volumes.json in the current directory; profiles/r10_time_volumes.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

import timing
from timing import REPS, ROOT, pkg, stats

F = np.float32
LATTICE = 33                                                            # points per axis of the sphere's lattice


def sphere_lattice(radius):
    h = 2.0 * radius / (LATTICE - 5)                                    # two spacings of margin on every side
    a = (np.arange(LATTICE) - 0.5 * (LATTICE - 1)) * h
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(F), F(h)


def boxes(state, K, dt):
    centres, r = timing.body_grid(state, K)
    values, h = sphere_lattice(r)
    half = F(0.5) * F(LATTICE - 1) * h
    out = []
    for c in centres:
        out.append(pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c, (half, half, half), rotation=(0.9, 0.1, 0.3, 0.2), vel=(0.02 * r / dt, 0.0, 0.0),
                                omega=(0.0, 0.5 / (16 * dt), 0.1 / (16 * dt))))
    return out, values, h


def engine(state, sp, stream, K, bound):
    f = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    obs, values, h = boxes(state, K, float(sp.param_timeStep))
    f.set_obstacles(obs)
    if bound:
        vid = f.create_volume(values, h)
        for k in range(K):
            f.bind_obstacle_volume(k, vid)
    return f


def obstacle_pass(state, sp, stream, K, bound):
    f = engine(state, sp, stream, K, bound)
    us = timing.other_per_dispatch(f)
    f.close()
    return stats(us)


def moved_fraction(state, sp, stream, K, bound):
    return timing.moved_fraction(state, sp, stream, engine(state, sp, stream, K, bound))


def icosphere(subdivisions):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import volume_ref
    return volume_ref.icosphere(subdivisions, 1.0)


def mesh_build(f, n, subdivisions):
    import torch
    v, t = icosphere(subdivisions)
    h = 2.9 / (n - 1)
    origin = (-1.45 + 0.0013, -1.45 + 0.0007, -1.45 + 0.0011)
    wall, dev = [], []
    for k in range(1 + 3):
        f.kernel_times(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f.mesh_distance(v, t, origin, h, (n, n, n))               # (synchronises the engine's stream)
        wall.append((time.perf_counter() - t0) * 1e6)
        dev.append(f.kernel_times(reset=True)["other"][0] * 1000.0)
    pairs = float(n) ** 3 * len(t)
    d = float(np.median(dev[1:]))
    return {"points": n ** 3, "triangles": int(len(t)), "pairs": pairs, "wall_us": stats(wall[1:]), "device_us": stats(dev[1:]),
            "pairs_per_second_device": pairs / (d * 1e-6), "inside_points": int((out < 0).sum().item())}


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "volumes")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    res = timing.header("tools/time_volumes.py", cfg, rec, variant_library=True, samples_per_case=REPS, volume_lattice=[LATTICE] * 3,
                        regimes={}, mesh_distance={})
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for label, n, sub in (("128^3 x 20480", 128, 5), ("64^3 x 1280", 64, 3)):
        res["mesh_distance"][label] = mesh_build(f, n, sub)
        print(label, json.dumps(res["mesh_distance"][label]), flush=True)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    for label, substep, state in timing.regimes(f, single_step_compute=True):
        yard = timing.copy_yardstick(len(state), stream)
        r = {"substep": substep, "yardstick": yard}
        for K in (1, 4):
            box, vol = obstacle_pass(state, sp, stream, K, False), obstacle_pass(state, sp, stream, K, True)
            r[f"K{K}"] = {"box_pass": box, "volume_pass": vol, "volume_over_box": vol["median_us"] / box["median_us"],
                          "volume_over_copy": vol["median_us"] / yard["median_us"], "box_over_copy": box["median_us"] / yard["median_us"],
                          "inside_box": moved_fraction(state, sp, stream, K, False), "inside_solid": moved_fraction(state, sp, stream, K, True)}
            print(label, K, json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r[f"K{K}"].items()}), "copy_us", yard["median_us"], flush=True)
        res["regimes"][label] = r
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
