"""Timing of the field sampler (include/sph_abi.h "field sampling") at config 3 (4 M particles, 128^3 cells, h = cellSize), on the
lattice state (substep 0) and after 300 substeps (the compressed regime):

  (a) a 256^3 lattice over the grid at spacing h/2, SPH_FIELD_DENSITY   (k_sample_lattice: LDS-staged bricks)
  (b) the same lattice, SPH_FIELD_ALL
  (c) (a)'s points through sph_sample_points_device                     (k_sample_points: the plain kernel; same bits as (b))
  (d) 1 M random probes inside the grid
  (e) the grid build every call runs first (a call with m = 0)

Device events on the engine's stream around each call, 3 warm-up calls, median and spread of 25.
  python tools/time_sample.py [out.json]
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd")


def main() -> None:
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_time_sample.json")
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    sp = pkg.default_params(**syn.params_fields(cfg))
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    g = f.ComputeGridExtents()
    h = sp.param_h
    spacing = (h / 2, h / 2, h / 2)
    dims = (2 * g.dims[0], 2 * g.dims[1], 2 * g.dims[2])
    npts = dims[0] * dims[1] * dims[2]
    origin = tuple(float(x) for x in g.gridMin)
    axes = [torch.tensor(np.float32(origin[a]) + np.arange(dims[a], dtype=np.float32) * np.float32(spacing[a]), device="cuda") for a in range(3)]
    Z, Y, X = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    lat_pts = torch.zeros((npts, 4), dtype=torch.float32, device="cuda")
    lat_pts[:, 0], lat_pts[:, 1], lat_pts[:, 2] = X.reshape(-1), Y.reshape(-1), Z.reshape(-1)
    del X, Y, Z
    rng = np.random.default_rng(7)
    lo = np.array(g.gridMin, np.float32)
    hi = lo + np.float32(g.cellSize) * np.array(g.dims, np.float32)
    rnd = np.zeros((1 << 20, 4), np.float32)
    rnd[:, :3] = lo + (hi - lo) * rng.random((1 << 20, 3))
    rnd_pts = torch.from_numpy(rnd).cuda()
    out_f = torch.empty(npts, dtype=torch.float32, device="cuda")
    out_all = torch.empty((npts, 8), dtype=torch.float32, device="cuda")
    out_pts = torch.empty((npts, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn, reps=25, warm=3):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b) * 1000.0)
        ms = np.array(ms)
        return {"median_us": float(np.median(ms)), "min_us": float(ms.min()), "max_us": float(ms.max()),
                "p10_us": float(np.percentile(ms, 10)), "p90_us": float(np.percentile(ms, 90)), "calls": int(reps)}

    res = {"tool": "tools/time_sample.py", "csrc_hash": pkg.build.csrc_hash(), "config": cfg.name, "particles": int(len(rec)),
           "grid": list(g.dims), "lattice": list(dims), "lattice_points": int(npts), "spacing": "h/2", "random_probes": 1 << 20,
           "device": torch.cuda.get_device_name(0), "regimes": {}}
    done = 0
    for label, substep in (("lattice_state", 0), ("compressed", 300)):
        if substep > done:
            f.DispatchN(substep - done)
            done = substep
        f.sync()
        r = {}
        r["a_lattice_density"] = timed(lambda: f.sample_lattice_device(origin, spacing, dims, out_f.data_ptr(), pkg.SPH_FIELD_DENSITY))
        r["b_lattice_all"] = timed(lambda: f.sample_lattice_device(origin, spacing, dims, out_all.data_ptr(), pkg.SPH_FIELD_ALL))
        r["c_points_plain_kernel"] = timed(lambda: f.sample_device(lat_pts.data_ptr(), npts, out_pts.data_ptr()))
        r["d_random_probes_1M"] = timed(lambda: f.sample_device(rnd_pts.data_ptr(), 1 << 20, out_pts.data_ptr()))
        r["e_grid_build"] = timed(lambda: f.sample_device(0, 0, 0))
        # the plain-kernel A/B must return the same bits as the staged lattice
        f.sample_lattice_device(origin, spacing, dims, out_all.data_ptr(), pkg.SPH_FIELD_ALL)
        f.sample_lattice_device(origin, spacing, dims, out_f.data_ptr(), pkg.SPH_FIELD_DENSITY)
        f.sample_device(lat_pts.data_ptr(), npts, out_pts.data_ptr())
        f.sync()
        r["c_equals_b_bitwise"] = bool(torch.equal(out_all.view(torch.int32), out_pts.view(torch.int32)))
        r["a_equals_c_density_bitwise"] = bool(torch.equal(out_f.view(torch.int32), out_pts[:, 0].contiguous().view(torch.int32)))
        cnt = out_pts[:, 3].contiguous().view(torch.int32)
        r["mean_neighbours_within_h"] = float(cnt.double().mean())
        b = r["e_grid_build"]["median_us"]
        for k in ("a_lattice_density", "b_lattice_all", "c_points_plain_kernel", "d_random_probes_1M"):
            r[k]["build_share"] = b / r[k]["median_us"]
        res["regimes"][label] = dict(substep=substep, **r)
        print(label, json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
