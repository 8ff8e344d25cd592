"""Timing of the adjoint of the neighbourhood sums (include/sph_abi.h "the adjoint of the neighbourhood sums") at config 3 (4 M particles,
128^3 cells, h = cellSize) after 1 substep and after 300 substeps (the compressed regime), R = h, C = 1, 4, 16, 64,
all in ONE process on ONE state.  Three families, each with three columns: the adjoint call, the forward call of the same shape, and
what the adjoint replaces written in torch:

  query[C]     sph_aggregate_adjoint_query over a lattice of 128 x 128 x 64 points across the grid's box (point -> particle) | sph_aggregate_query of
               the same points | query_neighbors(device=True) + zeros.index_add_(0, idx, g[recv])
  moments[C]   sph_aggregate_adjoint_particles with MOMENTS | sph_aggregate_particles with MOMENTS | radius_graph + index_add_ of
               g[recv, 0] + sum_a d_a g[recv, 1 + a], d = x[send] - x[recv]
  route[C]     sph_aggregate_route_particles | sph_aggregate_arg_particles (MAX) | zeros.view(-1).index_add_ over arg * C + c
`adjoint` and `forward` are the engine's own brackets (SPH_OPT_TIMING, class `other`: ids, binning, stage, walk), `grid_build` the bin +
scan + scatter classes of the same calls; `torch` is between device events on the torch stream (the engine works on that stream here),
`graph` the list build with its export and `reduce` the index_add_ alone, C = 1, 4, 16; a route that does not fit is `not_measured`.
`adjoint_over_forward` is the ratio of the medians.  No ratio is fixed in advance.

  python tools/time_aggregate_adjoint.py [out.json] [--trace CSV]
  python tools/time_aggregate_adjoint.py --trace-run          a short run for `rocprofv3 --kernel-trace --stats --output-format csv`: C = 16, the
                                                              compressed regime, three calls of each adjoint; --trace CSV adds its per-kernel
                                                              averages (binning, stage, walk) to the result as `kernel_trace`
Without an argument the result goes to time_aggregate_adjoint.json in the current directory; profiles/r31_time_aggregate_adjoint.json is
the committed record of the kernels in the tree.
"""
from __future__ import annotations

import csv
import ctypes as C
import json
import sys

import timing
from timing import pkg, series

CHANNELS = (1, 4, 16, 64)
ROUTE_CHANNELS = (1, 4, 16)
REPS = 7
ROUTE_REPS = 3
LATTICE = (128, 128, 64)
KERNELS = ("k_adjoint_bin", "k_scan_reduce", "k_scan_blocksums", "k_scan_apply", "k_adjoint_scatter", "k_adjoint_rank", "k_adjoint_stage", "k_aggregate_adjoint",
           "k_aggregate_route", "k_aggregate_arg", "k_aggregate_stage", "k_aggregate<", "k_neighbors_ids")
vp = C.c_void_p


def call(f, fn, *args):
    info = pkg.SphAggregateInfo()
    pkg.engine._check(fn(f._h, *args, C.byref(info)))


def lattice_points(f, torch, np):
    g = f.ComputeGridExtents()
    lo, ext = np.array(list(g.gridMin), np.float32), np.array(list(g.dims), np.float32) * np.float32(g.cellSize)
    ax = [lo[a] + ext[a] * (np.arange(LATTICE[a], dtype=np.float32) + np.float32(0.5)) / np.float32(LATTICE[a]) for a in range(3)]
    p = np.zeros((LATTICE[2], LATTICE[1], LATTICE[0], 4), np.float32)
    p[..., 0], p[..., 1], p[..., 2] = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    return torch.from_numpy(p.reshape(-1, 4)).cuda()


def cases(f, torch, rng, np, n, pts, h, c):
    """name -> (adjoint call, forward call, torch route or None) on fresh tensors of C = c."""
    L, m = f._L, int(pts.shape[0])
    rnd = lambda *shape: torch.from_numpy(rng.normal(0.0, 1.0, shape).astype(np.float32)).cuda()
    x, gq, gm, gr = rnd(n, c), rnd(m, c), rnd(n, 4, c), rnd(n, c)
    outn, outq, outm = torch.empty((n, c), dtype=torch.float32, device="cuda"), torch.empty((m, c), dtype=torch.float32, device="cuda"), \
        torch.empty((n, 4, c), dtype=torch.float32, device="cuda")
    arg = torch.empty((n, c), dtype=torch.int32, device="cuda")
    plain = pkg.aggregate_config(radius=h, channels=c)
    mom = pkg.aggregate_config(radius=h, channels=c, flags=pkg.SPH_AGGREGATE_MOMENTS)
    mx = pkg.aggregate_config(radius=h, channels=c, op=pkg.SPH_AGGREGATE_MAX)
    call(f, L.sph_aggregate_arg_particles, C.byref(mx), vp(x.data_ptr()), vp(outn.data_ptr()), None, vp(arg.data_ptr()))
    f.sync()
    pos = torch.from_numpy(np.ascontiguousarray(f.download()["pos"][:, :3])).cuda()

    def torch_query():
        off, idx = f.query_neighbors(pts, h, device=True)
        recv = torch.repeat_interleave(torch.arange(m, device="cuda"), off[1:] - off[:-1])
        return lambda: torch.zeros((n, c), dtype=torch.float32, device="cuda").index_add_(0, idx.to(torch.int64), gq[recv])

    def torch_moments():
        recv, send = f.radius_graph(h)
        d = pos[send] - pos[recv]
        return lambda: torch.zeros((n, c), dtype=torch.float32, device="cuda").index_add_(
            0, send, gm[recv, 0] + d[:, 0:1] * gm[recv, 1] + d[:, 1:2] * gm[recv, 2] + d[:, 2:3] * gm[recv, 3])

    def torch_route():
        won = arg >= 0
        at = (arg.to(torch.int64) * c + torch.arange(c, device="cuda")[None, :])[won]
        return lambda: torch.zeros(n * c, dtype=torch.float32, device="cuda").index_add_(0, at, gr[won])

    return {
        "query": (lambda: call(f, L.sph_aggregate_adjoint_query, C.byref(plain), vp(pts.data_ptr()), m, vp(gq.data_ptr()), vp(outn.data_ptr())),
                  lambda: call(f, L.sph_aggregate_query, C.byref(plain), vp(pts.data_ptr()), m, vp(x.data_ptr()), vp(outq.data_ptr()), None),
                  (lambda: f.query_neighbors(pts, h, device=True), torch_query)),
        "moments": (lambda: call(f, L.sph_aggregate_adjoint_particles, C.byref(mom), vp(gm.data_ptr()), vp(outn.data_ptr())),
                    lambda: call(f, L.sph_aggregate_particles, C.byref(mom), vp(x.data_ptr()), vp(outm.data_ptr()), None),
                    (lambda: f.radius_graph(h), torch_moments)),
        "route": (lambda: call(f, L.sph_aggregate_route_particles, C.byref(mx), vp(arg.data_ptr()), vp(gr.data_ptr()), vp(outn.data_ptr())),
                  lambda: call(f, L.sph_aggregate_arg_particles, C.byref(mx), vp(x.data_ptr()), vp(outn.data_ptr()), None, vp(arg.data_ptr())),
                  (None, torch_route)),
    }


def torch_columns(stream, graph, make):
    import torch
    res = {}
    try:
        with torch.cuda.stream(stream):
            if graph is not None:
                res["graph"] = timing.events(graph, stream, reps=ROUTE_REPS, warm=1)
            res["reduce"] = timing.events(make(), stream, reps=ROUTE_REPS, warm=1)
    except RuntimeError as err:
        res["not_measured"] = str(err).splitlines()[0][:200]
    torch.cuda.empty_cache()
    return res


def read_trace(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    key = name.split("(")[0].replace("void ", "").replace("sph::", "")
                    out[key] = {"calls": int(row.get("Calls", 0)), "average_us": float(row.get("AverageNs", "nan")) / 1000.0}
                    break
    return out


def main() -> None:
    import numpy as np
    import torch
    args = sys.argv[1:]
    trace_run = "--trace-run" in args
    trace = args[args.index("--trace") + 1] if "--trace" in args else None
    plain = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--trace")]
    out_path = timing.out_path(plain, "aggregate_adjoint")
    cfg3, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    n, h = len(rec), float(sp.param_h)
    rng = np.random.default_rng(1)
    with torch.cuda.stream(stream):
        pts = lattice_points(f, torch, np)
    if trace_run:
        f.DispatchN(300)
        f.sync()
        with torch.cuda.stream(stream):
            todo = cases(f, torch, rng, np, n, pts, h, 16)
        stream.synchronize()
        for name, (adjoint, forward, _) in todo.items():
            for _ in range(3):
                adjoint()
            f.sync()
        f.close()
        return
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    res = timing.header("tools/time_aggregate_adjoint.py", cfg3, rec, reps=REPS, route_reps=ROUTE_REPS, radius="h", query_points=int(pts.shape[0]), regimes={})
    for label, substep, state in timing.regimes(f, download=False):
        r = {}
        for c in CHANNELS:
            with torch.cuda.stream(stream):
                todo = cases(f, torch, rng, np, n, pts, h, c)
            stream.synchronize()
            for name, (adjoint, forward, (graph, make)) in todo.items():
                a, grid_us = series(f, adjoint, reps=REPS, warm=2)
                fw = series(f, forward, reps=REPS, warm=2)[0]
                v = {"adjoint": a, "forward": fw, "grid_build": grid_us, "adjoint_over_forward": a["median_us"] / fw["median_us"]}
                if c in ROUTE_CHANNELS:
                    v["torch"] = torch_columns(stream, graph, make)
                r.setdefault(name, {})[str(c)] = v
                print(label, name, "C", c, "adjoint", round(a["median_us"]), "forward", round(fw["median_us"]), "torch",
                      json.dumps({k: (round(t["median_us"]) if isinstance(t, dict) else t) for k, t in v.get("torch", {}).items()}), flush=True)
            del todo
            torch.cuda.empty_cache()
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    if trace:
        res["kernel_trace"] = dict(read_trace(trace), note="rocprofv3 --kernel-trace --stats of --trace-run: C = 16, compressed regime, averages per launch")
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
