"""Timing of the k nearest neighbours (include/sph_abi.h "k nearest neighbours") at config 3 (4 M particles, 128^3 cells, h = cellSize)
after 300 substeps (the compressed regime), for k = 8, 16, 32, 64 at R = h and R = 2h, the default kernel
(k_knn: the rows in LDS) and the selection kernel (SPH_OPT_KNN_VARIANT 1).

A build synchronises, so device events around a call would time the host as well.  The numbers are the engine's own brackets
(SPH_OPT_TIMING, class `other`, which holds nothing but the ids kernel and the kNN kernel during these calls; the neighbour lists' calls
hold ids, count, the three scan kernels and the fill), one series per case after warm-ups, all in ONE process on ONE state:

  knn[variant][R][k]      ids + k_knn / k_knn_select                 (variant 1: fewer calls, it is the slow yardstick; `calls` says how many)
  neighbors_build[R]      sph_neighbors_build at the same R (code of the parent commit): the same candidates, scanned twice, and
                          `total` entries written; knn_over_neighbors = the ratio of the medians, per k
  torch_route[R]          what the feature replaces: radius_graph(R), a gather of the positions, the squared distances and a per-row
                          sort (one stable sort by distance, one by row), cut at k = 16; device events on the torch stream around
                          the whole route (it includes the list build and its export)
  grid_build              bin + scan + scatter classes of the same calls (what every build runs first)

  python tools/time_knn.py [out.json]
Without an argument the result goes to time_knn.json in the current directory; profiles/r17_time_knn.json is the committed record of
the kernel in the tree (profiles/r17_time_knn_sorted_rows.json: an earlier version of k_knn, not in the tree).
"""
from __future__ import annotations

import json
import sys

import timing
from timing import knn_build as knn, neighbors_build as lists, pkg, series

KS = (8, 16, 32, 64)
SLOW_REPS = 3                                                                    # calls of the selection kernel per case (seconds each at k = 64)


def torch_route(f, pos, R, k):
    """The k nearest within R from the radius graph in torch: (idx (n, k), d2 (n, k)) padded with -1 / inf."""
    import torch
    g = f.radius_graph(R)
    recv, send = g[0], g[1]
    d = pos[recv] - pos[send]
    d2 = (d * d).sum(dim=1)
    o = torch.sort(d2, stable=True).indices                                       # by distance, then (stable) by row: rows ascending, distance ascending
    o = o[torch.sort(recv[o], stable=True).indices]
    recv, send, d2 = recv[o], send[o], d2[o]
    n = pos.shape[0]
    deg = torch.bincount(recv, minlength=n)
    start = torch.cumsum(deg, 0) - deg
    rank = torch.arange(recv.numel(), device=pos.device) - start[recv]
    keep = rank < k
    idx = torch.full((n, k), -1, dtype=torch.int64, device=pos.device)
    out = torch.full((n, k), float("inf"), dtype=torch.float32, device=pos.device)
    idx[recv[keep], rank[keep]] = send[keep]
    out[recv[keep], rank[keep]] = d2[keep]
    return idx, out


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path(sys.argv[1:], "knn")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    n = len(rec)
    h = sp.param_h
    res = timing.header("tools/time_knn.py", cfg, rec, reps=timing.REPS, slow_reps=SLOW_REPS, regimes={})
    for label, substep, state in timing.regimes(f, (("compressed", 300),)):
        pos = torch.from_numpy(np.ascontiguousarray(state["pos"][:, :3])).cuda()
        r = {}
        for name, R in (("R=h", h), ("R=2h", 2.0 * h)):
            v = {"knn": {"0": {}, "1": {}}}
            nb, grid_us = series(f, lambda: lists(f, R))
            info = f.neighbor_info()
            v["neighbors_build"] = dict(nb, total=int(info.total), mean_degree=info.total / n, max_count=int(info.maxCount))
            v["grid_build"] = grid_us
            for k in KS:
                for variant in (0, 1):
                    f.set_option(pkg.SPH_OPT_KNN_VARIANT, variant)
                    t, _ = series(f, lambda: knn(f, k, R), reps=SLOW_REPS if variant else timing.REPS, warm=1 if variant else 3)
                    ki = f.knn_info()
                    v["knn"][str(variant)][str(k)] = dict(t, total=int(ki.total), rows_full=int(ki.rowsFull),
                                                          knn_over_neighbors=t["median_us"] / nb["median_us"])
                f.set_option(pkg.SPH_OPT_KNN_VARIANT, 0)
                print(label, name, "k", k, json.dumps({vv: v["knn"][vv][str(k)]["median_us"] for vv in ("0", "1")}),
                      "neighbors_build", nb["median_us"], flush=True)
            # the torch route once per radius (k = 16); checked against the engine's rows where the distances do not tie
            def rows_equal(routed):
                e_idx = f.knn(16, R, device=True)[0]
                stream.synchronize()
                return dict(rows_equal_share=float((routed[0] == e_idx.to(torch.int64)).all(dim=1).float().mean()))
            v["torch_route_k16"] = route = timing.torch_route(lambda: torch_route(f, pos, R, 16), rows_equal, stream, SLOW_REPS)
            if "not_measured" not in route:
                v["torch_route_over_knn_k16"] = route["median_us"] / v["knn"]["0"]["16"]["median_us"]
            print(label, name, "torch route", json.dumps(v["torch_route_k16"]), flush=True)
            r[name] = v
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
