"""Timing of ray spans (include/sph_abi.h "ray spans") against the first-hit cast of the same rays, at config 3 (4 M particles, 128^3
cells, h = cellSize) after 300 substeps (the compressed regime): the 1 M rays of tools/time_rays.py -- a
1024 x 1024 sheet straight down from above the grid's box, a 1024 x 1024 pinhole fan from a corner of it, uniformly random segments
between points of the box -- at r = h / 4 and r = h / 2, rays already in device memory.

The numbers are the engine's own brackets (SPH_OPT_TIMING, class `other`, which holds nothing but the kernels of a call during these
calls), one series per case after warm-ups, all in ONE process on ONE state:

  spans[kind][r][walk][order]   walk: layer (SPH_OPT_RAY_SPANS_VARIANT 0) or block (1); order: caller (SPH_OPT_RAYS_VARIANT 0: k_ray_spans
                                alone) or cell (1: k_rays_bin, the scan, k_rays_order and k_ray_spans); crossed rays, the sum of the
                                counts and the largest count of the case beside them
  cast[kind][r][order]          sph_rays_cast_device, first hit, of the same rays on the same state: the yardstick
  copy                          the plain device copy the other tools use (two float4 per particle)

  python tools/time_ray_spans.py [out.json]
Without an argument the result goes to time_ray_spans.json in the current directory; profiles/r24_time_ray_spans.json is the committed
record.
"""
from __future__ import annotations

import functools
import json
import sys

import timing
from timing import pkg

REPS = 6
SIDE = 1024
series = functools.partial(timing.series, reps=REPS, warm=2)
ORDERS = (("caller_order", 0), ("cell_order", 1))


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path(sys.argv[1:], "ray_spans")
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
    res = timing.header("tools/time_ray_spans.py", cfg, rec, reps=REPS, rays=SIDE * SIDE, regimes={})
    for label, substep, _ in timing.regimes(f, (("compressed", 300),), download=False):
        r = {"spans": {}, "cast": {}}
        for kind, rays in kinds.items():
            dev = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
            r["spans"][kind], r["cast"][kind] = {}, {}
            for rname, radius in (("r=h/4", 0.25 * h), ("r=h/2", 0.5 * h)):
                v, c = {}, {}
                for oname, order in ORDERS:
                    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, order)
                    c[oname], _ = series(f, lambda: timing.rays_cast(f, dev, radius, 0))
                    c[oname]["hits"] = int(f.rays_info().hits)
                    for wname, walk in (("layer_walk", 0), ("block_walk", 1)):
                        f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, walk)
                        t, _ = series(f, lambda: timing.rays_span(f, dev, radius))
                        info = f.ray_spans_info()
                        v.setdefault(wname, {})[oname] = dict(t, crossed=int(info.crossed), total=int(info.total), max_count=int(info.maxCount))
                f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 0)
                f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, 0)
                r["spans"][kind][rname], r["cast"][kind][rname] = v, c
                print(label, kind, rname, json.dumps({"cast": {o: c[o]["median_us"] for o in c}, **{w: {o: v[w][o]["median_us"] for o in v[w]} for w in v}}),
                      "crossed", v["layer_walk"]["caller_order"]["crossed"], "total", v["layer_walk"]["caller_order"]["total"], flush=True)
            del dev
        res["regimes"][label] = dict(substep=substep, **r)
    res["copy"] = timing.copy_yardstick(len(rec), stream)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
