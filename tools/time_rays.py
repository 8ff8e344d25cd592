"""Timing of ray casts against the particles (include/sph_abi.h "ray casts") at config 3 (4 M particles, 128^3 cells, h = cellSize) after
300 substeps (the compressed regime): 1 M rays of three kinds -- a 1024 x 1024 sheet straight down from above the
grid's box, a 1024 x 1024 pinhole fan from a corner of it, uniformly random segments between points of the box -- first hit and
SPH_RAYS_ANY_HIT, at r = h / 4 and r = h / 2, rays already in device memory (sph_rays_cast_device).

A cast synchronises, so device events around a call would time the host as well.  The numbers are the engine's own brackets
(SPH_OPT_TIMING, class `other`, which holds nothing but the kernels of a cast during these calls; for the kNN yardstick the ids kernel and k_knn), one
series per case after warm-ups, all in ONE process on ONE state:

  rays[kind][r][mode]     k_rays (the default: rays cast in the caller's order); hits and void rays of the case beside it; cell_order:
                          k_rays_bin, the scan, k_rays_order and k_rays under SPH_OPT_RAYS_VARIANT 1 (rays cast in the order of their cell of entry)
  grid_build              bin + scan + scatter classes of the same calls (what every cast runs first), shown separately
  knn_query_k8_R=h        sph_knn_query for 1 M points (the segments' start points), k = 8, R = h: the nearest yardstick among the queries
  copy                    the plain device copy the other tools use (two float4 per particle)

  python tools/time_rays.py [out.json]
Without an argument the result goes to time_rays.json in the current directory; profiles/r18_time_rays.json is the committed record.
"""
from __future__ import annotations

import functools
import json
import sys

import timing
from timing import pkg, rays_cast as cast

REPS = 10
SIDE = 1024
series = functools.partial(timing.series, reps=REPS, warm=2)


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path(sys.argv[1:], "rays")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    h = float(sp.param_h)
    g = pkg.compute_grid_extents(sp)
    lo = np.array(list(g.gridMin), np.float64)
    ext = np.array(list(g.dims), np.float64) * float(g.cellSize)
    rng = np.random.default_rng(18)
    a, b = lo + rng.random((SIDE * SIDE, 3)) * ext, lo + rng.random((SIDE * SIDE, 3)) * ext
    seg = np.zeros((SIDE * SIDE, 8), np.float32)
    seg[:, 0:3], seg[:, 4:7], seg[:, 7] = a, b - a, 1.0
    kinds = {
        "sheet_down": pkg.parallel_rays((lo[0], lo[1] + ext[1] + 1.0, lo[2]), (ext[0], 0, 0), (0, 0, ext[2]), (0, -1, 0), SIDE, SIDE),
        "fan_from_corner": pkg.camera_rays(lo + ext * 1.05, lo + ext * 0.5, (0, 1, 0), 1.0, SIDE, SIDE),
        "random_segments": seg,
    }
    res = timing.header("tools/time_rays.py", cfg, rec, reps=REPS, rays=SIDE * SIDE, regimes={})
    for label, substep, _ in timing.regimes(f, (("compressed", 300),), download=False):
        r = {"rays": {}}
        for kind, rays in kinds.items():
            dev = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
            r["rays"][kind] = {}
            for rname, radius in (("r=h/4", 0.25 * h), ("r=h/2", 0.5 * h)):
                v = {}
                for mode, flags in (("first_hit", 0), ("any_hit", pkg.SPH_RAYS_ANY_HIT)):
                    t, build = series(f, lambda: cast(f, dev, radius, flags))
                    info = f.rays_info()
                    v[mode] = dict(t, hits=int(info.hits), void_rays=int(info.voidRays), grid_build=build)
                    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 1)
                    v[mode]["cell_order"], _ = series(f, lambda: cast(f, dev, radius, flags))
                    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 0)
                r["rays"][kind][rname] = v
                print(label, kind, rname, json.dumps({m: (v[m]["median_us"], v[m]["cell_order"]["median_us"]) for m in v}), "hits", v["first_hit"]["hits"],
                      "grid build", v["first_hit"]["grid_build"]["median_us"], flush=True)
            del dev
        pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([seg[:, 0:3], np.zeros((len(seg), 1), np.float32)], axis=1))).cuda()
        knn, build = series(f, lambda: timing.knn_query(f, pts, 8, h))
        r["knn_query_k8_R=h"] = dict(knn, total=int(f.knn_info().total), grid_build=build)
        print(label, "knn query", knn["median_us"], flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    res["copy"] = timing.copy_yardstick(len(rec), stream)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
