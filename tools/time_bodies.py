"""Timing of dynamic rigid bodies and of the lattice moments (include/sph_abi.h "dynamic rigid bodies"), protocol
of tools/time_obstacles.py: config 3 (4 M particles, 128^3 cells), device events (SPH_OPT_TIMING, class `other`: the bracket around the
obstacle pass and its finish), 25 substeps after 3 warm-ups, median [p10, p90].

  kinematic     the obstacle step with K = 4 kinematic bodies and no dynamics record: the same kernels as before this feature.  With
                --parent-tree DIR (a built checkout of the parent commit) the same measurement runs from that tree too, in child
                processes that alternate between the two trees, ROUNDS times each: the difference of the medians has to sit inside the
                spread of the parent's own repeats.
  dynamic       the same bodies, all four with a dynamics record (k_obstacles_finish_dyn instead of k_obstacles_finish).
  moments       sph_volume_moments on lattices of 128^3, 256^3 and 512^3 points: device time of the two kernels, bytes of lattice read
                per second, and that rate over the float4-copy rate of the device (6.29 TB/s measured on MI355X).
  --trace CSV   per-kernel averages of a `rocprofv3 --kernel-trace --stats --output-format csv` run of `--trace-run` (a short run with
                kinematic and dynamic sets and one moments call) are copied into the result: the one-block finish kernels are too short
                for the bracket to tell apart.
  python tools/time_bodies.py [out.json] [--parent-tree DIR] [--trace CSV]
Without an out.json the result goes to time_bodies.json in the current directory; profiles/r11_time_bodies.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import csv
import json
import os
import subprocess
import sys

import numpy as np

import timing
from timing import HERE, REPS, ROOT, pkg, stats                         # ROOT: the tree SPH_TREE names (child processes), else HERE

F = np.float32
ROUNDS = 3
COPY_BYTES_PER_S = 6.29e12
KERNELS = ("k_obstacles_finish_dyn", "k_obstacles_finish", "k_obstacles", "k_volume_moments_finish", "k_volume_moments")


def bodies(state, dt, K=4):
    centres, r = timing.body_grid(state, K)
    out = []
    for k, c in enumerate(centres):
        shape = k % 3
        size = (r,) if shape == 0 else ((r, 0.8 * r, 0.6 * r) if shape == 1 else (0.6 * r, 0.7 * r))
        out.append(pkg.obstacle(shape, c, size, rotation=(0.9, 0.1, 0.3, 0.2), vel=(0.02 * r / dt, 0.0, 0.0), omega=(0.0, 0.5 / (16 * dt), 0.1 / (16 * dt))))
    return out, r


def obstacle_step(rec, sp, stream, dynamic):
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    obs, r = bodies(rec, float(sp.param_timeStep))
    f.set_obstacles(obs)
    if dynamic:
        rho = float(sp.param_restDensity)
        for k, o in enumerate(obs):
            make = (pkg.dynamics_sphere, pkg.dynamics_box, pkg.dynamics_capsule)[o.shape]
            f.set_obstacle_dynamics(k, make(0.6 * rho, list(o.size)[:3] if o.shape else o.size[0]))
    us = timing.other_per_dispatch(f)
    f.close()
    return stats(us)


def kinematic_child(out_path):
    """Child process: the kinematic obstacle step from the tree SPH_TREE names (only what the parent commit has is used)."""
    import torch
    _, rec, sp = timing.config3()
    res = obstacle_step(rec, sp, torch.cuda.Stream(), False)
    res["tree"] = ROOT
    res["csrc_hash"] = pkg.build.csrc_hash()
    with open(out_path, "w") as fh:
        json.dump(res, fh)


def sphere_lattice(n):
    h = 2.0 / (n - 1)
    a = (np.arange(n) - 0.5 * (n - 1)) * h
    z, y, x = np.meshgrid(a.astype(F), a.astype(F), a.astype(F), indexing="ij", sparse=True)
    return (np.sqrt(x * x + y * y + z * z) - F(0.8)).astype(F), h


def moments(f, n):
    values, h = sphere_lattice(n)
    vid = f.create_volume(values, h)
    dev = []
    for _ in range(3 + 10):
        f.kernel_times(reset=True)
        m = f.volume_moments(vid)
        dev.append(f.kernel_times(reset=True)["other"][0] * 1000.0)
    f.destroy_volume(vid)
    d = stats(dev[3:])
    rate = values.size * 4 / (d["median_us"] * 1e-6)
    return {"points": int(values.size), "device_us": d, "bytes_per_second": rate, "over_float4_copy": rate / COPY_BYTES_PER_S,
            "volume": float(m[0]), "analytic_volume": 4.0 / 3.0 * np.pi * 0.8 ** 3}


def trace_run():
    """A short run for a kernel trace: 40 substeps kinematic, 40 dynamic, moments of a 256^3 lattice."""
    import torch
    _, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    for dynamic in (False, True):
        f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
        obs, _ = bodies(rec, float(sp.param_timeStep))
        f.set_obstacles(obs)
        if dynamic:
            for k in range(len(obs)):
                f.set_obstacle_dynamics(k, pkg.dynamics_sphere(0.6 * float(sp.param_restDensity), 1.0))
        f.DispatchN(40)
        f.download()
        if dynamic:
            values, h = sphere_lattice(256)
            vid = f.create_volume(values, h)
            for _ in range(10):
                f.volume_moments(vid)
        f.close()


def read_trace(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for k in KERNELS:
                if name.startswith(k + "(") or name == k or name.startswith("sph::" + k + "(") or name.startswith("void sph::" + k):
                    out[k] = {"calls": int(row.get("Calls", 0)), "average_us": float(row.get("AverageNs", "nan")) / 1000.0,
                              "min_us": float(row.get("MinNs", "nan")) / 1000.0, "max_us": float(row.get("MaxNs", "nan")) / 1000.0}
                    break
    return out


def main() -> None:
    args = sys.argv[1:]
    if args and args[0] == "--kinematic":
        return kinematic_child(args[1])
    if args and args[0] == "--trace-run":
        return trace_run()
    import torch
    parent = args[args.index("--parent-tree") + 1] if "--parent-tree" in args else None
    trace = args[args.index("--trace") + 1] if "--trace" in args else None
    plain = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--parent-tree", "--trace"))]
    out_path = timing.out_path(plain, "bodies")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    res = timing.header("tools/time_bodies.py", cfg, rec, samples_per_case=REPS, bodies=4)
    res["kinematic"] = obstacle_step(rec, sp, stream, False)
    res["dynamic"] = obstacle_step(rec, sp, stream, True)
    res["dynamic_minus_kinematic_us"] = res["dynamic"]["median_us"] - res["kinematic"]["median_us"]
    print("kinematic", res["kinematic"]["median_us"], "dynamic", res["dynamic"]["median_us"], flush=True)
    f = pkg.SPHFluidGPU.from_particles(rec[:4096], sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    res["moments"] = {f"{n}^3": moments(f, n) for n in (128, 256, 512)}
    f.close()
    print("moments", json.dumps({k: (v["device_us"]["median_us"], v["over_float4_copy"]) for k, v in res["moments"].items()}), flush=True)
    if parent:
        runs = {"this": [], "parent": []}
        tmp = out_path + ".child.json"
        for _ in range(ROUNDS):
            for label, tree in (("parent", parent), ("this", HERE)):
                env = dict(os.environ, SPH_TREE=os.path.abspath(tree))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--kinematic", tmp], check=True, env=env, timeout=600)
                with open(tmp) as fh:
                    runs[label].append(json.load(fh))
        os.remove(tmp)
        med = {k: [r["median_us"] for r in v] for k, v in runs.items()}
        res["kinematic_against_parent"] = {"rounds": ROUNDS, "interleaved": True, "this_median_us": med["this"], "parent_median_us": med["parent"],
                                           "parent_spread_us": max(med["parent"]) - min(med["parent"]),
                                           "difference_of_medians_us": float(np.median(med["this"]) - np.median(med["parent"])),
                                           "parent_csrc_hash": runs["parent"][0]["csrc_hash"], "runs": runs}
        print("against parent", json.dumps({k: v for k, v in res["kinematic_against_parent"].items() if k != "runs"}), flush=True)
    if trace:
        res["kernel_trace"] = read_trace(trace)
        print("trace", json.dumps(res["kernel_trace"]), flush=True)
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
