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
Without an argument the result goes to time_surface.json in the current directory; profiles/r06_time_surface.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys
import time

import numpy as np

import timing
from timing import pkg, stats


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "surface")
    cfg, rec, sp = timing.config3()
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
        return stats(us)

    res = timing.header("tools/time_surface.py", cfg, rec, grid=list(g.dims), lattice=list(dims), lattice_points=int(npts), spacing="h/2",
                        field="fraction", iso=0.5, regimes={})
    # substep 0: the spawned records carry no density yet, so the fraction is 0 everywhere and the mesh is empty (count and scan only)
    for label, substep, _ in timing.regimes(f, (("spawned_empty", 0),) + timing.REGIMES, download=False):
        r = {}
        r["a_sample_fraction"] = timing.events(lambda: f.sample_lattice_device(origin, spacing, dims, vol.data_ptr(), pkg.SPH_FIELD_FRACTION),
                                               stream, reps, warm)
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
        r["b_mesher_kernels"] = dict(stats(kus), launches_per_call=int(np.median(launches)))
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
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
