"""Timing of the iso-surface mesher (include/sph_abi.h "iso-surface") at BASELINE.json configs[2] (4 M
particles, 128^3 cells, h = cellSize) on the 256^3 lattice of spacing h/2 over the grid, SPH_FIELD_FRACTION, iso 0.5, on the lattice
state (after 1 substep; at substep 0 the records carry no density and the fraction is 0 everywhere, an empty mesh, also recorded)
and after 300 substeps (the compressed regime):

  (a) the sampling that feeds the mesher: sph_sample_lattice of the fraction (grid build + k_sample_lattice), device events
  (b) the mesher alone on that volume: sph_extract_surface_volume; its four kernels' device time (SPH_OPT_TIMING, class "other":
      k_surf_count, k_surf_scan_tiles, k_surf_vertices, k_surf_triangles) and the wall time of the call, which waits once for the
      counts
  (c) sph_extract_surface: (a) and (b) in one call, wall time
  plus vertex and triangle counts and the bytes of the mesh (24 per vertex, 12 per triangle).

3 warm-up calls, median and spread of 25.
  python tools/time_surface.py [out.json]
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
pkg = importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd")


def _stats(us):
    us = np.array(us)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
            "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "calls": int(len(us))}


def main() -> None:
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_time_surface.json")
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
    vol = torch.empty(npts, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    reps, warm = 25, 3

    def events(fn):
        for _ in range(warm):
            fn()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            us.append(a.elapsed_time(b) * 1000.0)
        return _stats(us)

    def wall(fn):
        for _ in range(warm):
            fn()
            f.sync()
        us = []
        for _ in range(reps):
            f.sync()
            t0 = time.perf_counter()
            fn()
            f.sync()
            us.append((time.perf_counter() - t0) * 1e6)
        return _stats(us)

    res = {"tool": "tools/time_surface.py", "csrc_hash": pkg.build.csrc_hash(), "config": cfg.name, "particles": int(len(rec)),
           "grid": list(g.dims), "lattice": list(dims), "lattice_points": int(npts), "spacing": "h/2", "field": "fraction", "iso": 0.5,
           "device": torch.cuda.get_device_name(0), "regimes": {}}
    done = 0
    # substep 0: the spawned records carry no density yet, so the fraction is 0 everywhere and the mesh is empty (count and scan only)
    for label, substep in (("spawned_empty", 0), ("lattice_state", 1), ("compressed", 300)):
        if substep > done:
            f.DispatchN(substep - done)
            done = substep
        f.sync()
        r = {}
        r["a_sample_fraction"] = events(lambda: f.sample_lattice_device(origin, spacing, dims, vol.data_ptr(), pkg.SPH_FIELD_FRACTION))
        f.sync()
        # (b) the mesher's kernels: device time of class "other" per call, and the call's wall time
        f.set_option(pkg.SPH_OPT_TIMING, 1)
        for _ in range(warm):
            f.extract_surface_volume(vol.data_ptr(), origin, spacing, dims, 0.5)
        f.sync()
        f.kernel_times(reset=True)
        kus, launches = [], []
        for _ in range(reps):
            f.extract_surface_volume(vol.data_ptr(), origin, spacing, dims, 0.5)
            f.sync()
            kt = f.kernel_times(reset=True)
            kus.append(kt["other"][0] * 1000.0)
            launches.append(int(kt["other"][1]))
        f.set_option(pkg.SPH_OPT_TIMING, 0)
        r["b_mesher_kernels"] = dict(_stats(kus), launches_per_call=int(np.median(launches)))
        r["b_mesher_call_wall"] = wall(lambda: f.extract_surface_volume(vol.data_ptr(), origin, spacing, dims, 0.5))
        r["c_extract_surface_wall"] = wall(lambda: f.extract_surface(origin, spacing, dims, 0.5, pkg.SPH_FIELD_FRACTION))
        surf = f.extract_surface(origin, spacing, dims, 0.5, pkg.SPH_FIELD_FRACTION)
        f.sync()
        v, t = f._download_surface(surf)
        r["vertices"] = int(surf.numVertices)
        r["triangles"] = int(surf.numTriangles)
        r["mesh_bytes"] = int(24 * surf.numVertices + 12 * surf.numTriangles)
        r["mesher_over_sampling"] = r["b_mesher_kernels"]["median_us"] / r["a_sample_fraction"]["median_us"]
        r["sampled_volume_nonzero"] = int(torch.count_nonzero(vol))
        # the same bits through the volume path (the sampled path meshes exactly what sph_sample_lattice writes)
        v2, t2 = f.surface_from_volume(vol.data_ptr(), origin, spacing, dims, 0.5)
        r["sampled_equals_volume_bitwise"] = bool(v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes())
        res["regimes"][label] = dict(substep=substep, **r)
        print(label, json.dumps({k: (x["median_us"] if isinstance(x, dict) else x) for k, x in r.items()}), flush=True)
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
