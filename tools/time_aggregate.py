"""Timing of the fused neighbourhood reductions (include/sph_abi.h "fused neighbourhood reductions") at config 3 (4 M particles, 128^3
cells, h = cellSize) after 1 substep and after 300 substeps (the compressed regime), R = h, C = 1, 4, 16, 64, for
SUM, MEAN and SUM with MOMENTS, all in ONE process on ONE state:

  aggregate[op][C][variant]   the engine's own brackets (SPH_OPT_TIMING, class `other`: ids, the stage where there is one, the walk) of
                              sph_aggregate_particles on a device tensor, per value of SPH_OPT_AGGREGATE_VARIANT: "staged" (0, the
                              default), "by_id" (1), "chunk4" / "chunk8" / "chunk16" (2 / 4 / 6, staged) and, where C % 4 == 0,
                              "loads4B" (8: 4-byte payload loads); `fused_over_neighbors` = the default's median over neighbors_build's
  neighbors_build             sph_neighbors_build at the same radius: the same walk twice (count, fill) plus the scan, and `total`
                              indices written; the yardstick of the walk without a payload
  grid_build                  bin + scan + scatter classes of the same calls (what every query runs first)
  torch_route[C]              what the fused call replaces, C = 1, 4, 16: zeros.index_add_(0, recv, x[send] - x[recv]) over
                              radius_graph(R), device events on the torch stream (the engine works on that stream here): `graph` the
                              list build with its export and the edge list, `reduce` the gather and the index_add_ alone, and `fused`
                              the fused SUM with DELTA between the same events (grid build included, as `graph` includes it);
                              `fused_over_route` = fused / (graph + reduce), and the largest difference of the fused result from the
                              route's and from a float64 index_add_ taken in eight slices of the edges

  python tools/time_aggregate.py [out.json]
Without an argument the result goes to time_aggregate.json in the current directory; profiles/r30_time_aggregate.json is the committed
record of the kernels in the tree.
"""
from __future__ import annotations

import ctypes as C
import json
import sys

import timing
from timing import neighbors_build as lists, pkg, series

CHANNELS = (1, 4, 16, 64)
ROUTE_CHANNELS = (1, 4, 16)
REPS = 9                                                                           # calls per case (tens of milliseconds each at C = 64)
ROUTE_REPS = 3
CASES = (("sum", pkg.SPH_AGGREGATE_SUM, 0), ("mean", pkg.SPH_AGGREGATE_MEAN, 0), ("sum_moments", pkg.SPH_AGGREGATE_SUM, pkg.SPH_AGGREGATE_MOMENTS))
VARIANTS = (("staged", 0), ("by_id", 1), ("chunk4", 2), ("chunk8", 4), ("chunk16", 6), ("loads4B", 8))


def fused(f, cfg, x, out):
    """sph_aggregate_particles through the C ABI alone, on device tensors (no synchronisation)."""
    info = pkg.SphAggregateInfo()
    pkg.engine._check(f._L.sph_aggregate_particles(f._h, C.byref(cfg), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), None, C.byref(info)))
    return info


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path(sys.argv[1:], "aggregate")
    cfg3, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    n = len(rec)
    h = float(sp.param_h)
    res = timing.header("tools/time_aggregate.py", cfg3, rec, reps=REPS, route_reps=ROUTE_REPS, radius="h", regimes={})
    rng = np.random.default_rng(1)
    for label, substep, state in timing.regimes(f):
        r = {"aggregate": {}, "torch_route": {}}
        nb, grid_us = series(f, lambda: lists(f, h))
        info = f.neighbor_info()
        r["neighbors_build"] = dict(nb, total=int(info.total), mean_degree=info.total / n, max_count=int(info.maxCount))
        r["grid_build"] = grid_us
        for c in CHANNELS:
            with torch.cuda.stream(stream):
                x = torch.from_numpy(rng.normal(0.0, 1.0, (n, c)).astype(np.float32)).cuda()
                out = torch.empty((n, 4, c), dtype=torch.float32, device="cuda")
            stream.synchronize()
            for name, op, flags in CASES:
                cfg = pkg.aggregate_config(radius=h, op=op, flags=flags, channels=c)
                v = {}
                for vname, variant in VARIANTS:
                    if vname == "loads4B" and c % 4:
                        continue
                    f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, variant)
                    v[vname] = series(f, lambda: fused(f, cfg, x, out), reps=REPS, warm=2)[0]
                f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, 0)
                v["fused_over_neighbors"] = v["staged"]["median_us"] / nb["median_us"]
                r["aggregate"].setdefault(name, {})[str(c)] = v
                print(label, name, "C", c, json.dumps({k: round(t["median_us"]) for k, t in v.items() if isinstance(t, dict)}),
                      "neighbors_build", round(nb["median_us"]), flush=True)
            if c in ROUTE_CHANNELS:
                r["torch_route"][str(c)] = route(f, stream, x, out, h, c)
                print(label, "torch route C", c, json.dumps(r["torch_route"][str(c)]), flush=True)
            del x, out
            torch.cuda.empty_cache()
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


def route(f, stream, x, out, h, c):
    """README's route against the fused SUM with DELTA, both between device events on the one stream."""
    import torch
    cfg = pkg.aggregate_config(radius=h, flags=pkg.SPH_AGGREGATE_DELTA, channels=c)
    res = {}
    try:
        with torch.cuda.stream(stream):
            res["fused"] = timing.events(lambda: fused(f, cfg, x, out), stream, reps=ROUTE_REPS, warm=1)
            res["graph"] = timing.events(lambda: f.radius_graph(h), stream, reps=ROUTE_REPS, warm=1)
            g = f.radius_graph(h)
            recv, send = g[0], g[1]
            reduce = lambda: torch.zeros_like(x).index_add_(0, recv, x[send] - x[recv])
            res["reduce"] = timing.events(reduce, stream, reps=ROUTE_REPS, warm=1)
            res["edges"] = int(recv.numel())
            fused(f, cfg, x, out)
            f.sync()
            got = out.view(-1)[:x.numel()].view_as(x)
            res["max_abs_difference"] = float((reduce() - got).abs().max())
            ref = torch.zeros(x.shape, dtype=torch.float64, device=x.device)            # the same sum in float64, the edges in eight slices
            for s in torch.arange(recv.numel(), device=x.device).chunk(8):
                ref.index_add_(0, recv[s], (x[send[s]] - x[recv[s]]).double())
            res["max_abs_difference_float64_slices"] = float((ref - got.double()).abs().max())
            res["fused_over_route"] = res["fused"]["median_us"] / (res["graph"]["median_us"] + res["reduce"]["median_us"])
    except RuntimeError as err:
        res["not_measured"] = str(err).splitlines()[0][:200]
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
