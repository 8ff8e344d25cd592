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
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd")
from time_obstacles import REPS, copy_yardstick, other_us, stats  # noqa: E402

F = np.float32
LATTICE = 33                                                            # points per axis of the sphere's lattice


def sphere_lattice(radius):
    h = 2.0 * radius / (LATTICE - 5)                                    # two spacings of margin on every side
    a = (np.arange(LATTICE) - 0.5 * (LATTICE - 1)) * h
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(F), F(h)


def boxes(state, K, dt):
    fluid = state["pos"][state["isGhost"] == 0][:, :3].astype(np.float64)
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    side = int(np.ceil(K ** (1.0 / 3.0) - 1e-9))
    cell = (hi - lo) / side
    r = 0.3 * float(cell.min())
    values, h = sphere_lattice(r)
    half = F(0.5) * F(LATTICE - 1) * h
    out = []
    for k in range(K):
        i, j, l = k % side, (k // side) % side, k // (side * side)
        c = lo + cell * (np.array([i, j, l]) + 0.5)
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
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(3):
        f.DispatchCompute()
    other_us(f)
    us = []
    for _ in range(REPS):
        f.DispatchCompute()
        t, launches = other_us(f)
        assert launches == 1, launches
        us.append(t)
    f.close()
    return stats(us)


def moved_fraction(state, sp, stream, K, bound):
    a, b = engine(state, sp, stream, K, bound), pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    a.DispatchCompute()
    b.DispatchCompute()
    ra, rb = a.download(), b.download()
    a.close()
    b.close()
    return float((ra["pos"] != rb["pos"]).any(axis=1).mean())


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_time_volumes.json")
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    sp = pkg.default_params(**syn.params_fields(cfg))
    stream = torch.cuda.Stream()
    res = {"tool": "tools/time_volumes.py", "csrc_hash": pkg.build.csrc_hash(), "library": os.path.basename(os.environ.get("SPH_HIP_LIB") or "libsph_hip.so"),
           "config": cfg.name, "particles": int(len(rec)), "device": torch.cuda.get_device_name(0), "samples_per_case": REPS,
           "volume_lattice": [LATTICE] * 3, "regimes": {}, "mesh_distance": {}}
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for label, n, sub in (("128^3 x 20480", 128, 5), ("64^3 x 1280", 64, 3)):
        res["mesh_distance"][label] = mesh_build(f, n, sub)
        print(label, json.dumps(res["mesh_distance"][label]), flush=True)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    done = 0
    for label, substep in (("lattice_state", 1), ("compressed", 300)):
        f.DispatchN(substep - done) if substep - done > 1 else f.DispatchCompute()
        done = substep
        state = f.download()
        yard = copy_yardstick(len(state), stream)
        r = {"substep": substep, "yardstick": yard}
        for K in (1, 4):
            box, vol = obstacle_pass(state, sp, stream, K, False), obstacle_pass(state, sp, stream, K, True)
            r[f"K{K}"] = {"box_pass": box, "volume_pass": vol, "volume_over_box": vol["median_us"] / box["median_us"],
                          "volume_over_copy": vol["median_us"] / yard["median_us"], "box_over_copy": box["median_us"] / yard["median_us"],
                          "inside_box": moved_fraction(state, sp, stream, K, False), "inside_solid": moved_fraction(state, sp, stream, K, True)}
            print(label, K, json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r[f"K{K}"].items()}), "copy_us", yard["median_us"], flush=True)
        res["regimes"][label] = r
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
