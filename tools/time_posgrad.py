"""Timing of the position gradients of the neighbourhood sums (include/sph_abi.h "position gradients of the neighbourhood sums") at config 3
(4 M particles, 128^3 cells, h = cellSize) after 1 substep and after 300 substeps (the compressed regime), R = h,
the poly6 weight, C = 1, 16, 64, all in ONE process on ONE state.  Three families:

  particles[C]   sph_aggregate_posgrad_particles | the forward sph_aggregate_particles | the adjoint sph_aggregate_adjoint_particles |
                 the torch route
  moments[C]     the same three engine calls with MOMENTS (no torch route: its four planes per pair do not fit beside the rest)
  query[C]       sph_aggregate_posgrad_query with both outputs from a lattice of 128 x 128 x 64 points across the grid's box | with the
                 points' output alone | with the particles' output alone | sph_aggregate_query | sph_aggregate_adjoint_query | the torch route
The engine's columns are its own brackets (SPH_OPT_TIMING, class `other`: ids, binning, stages, walks), `grid_build` the bin + scan +
scatter classes of the posgrad call.  The torch route is what a user writes without these calls: radius_graph (or query_neighbors) for
the pairs, a gather of the values, the weights (R^2 - r^2)^3 from a positions tensor that requires grad, index_add_ into the rows and
backward() of sum(out * g); `graph` is the list build with its export, `loss` everything after it, between device events on the torch
stream (the engine works on that stream here), C = 1 and 16; a route that does not fit is `not_measured`.  No ratio is fixed in advance.

  python tools/time_posgrad.py [out.json]
Without an argument the result goes to time_posgrad.json in the current directory; profiles/r33_time_posgrad.json is the committed record
of the kernels in the tree.
"""
from __future__ import annotations

import ctypes as C
import json
import sys

import timing
from timing import pkg, series

CHANNELS = (1, 16, 64)
TORCH_CHANNELS = (1, 16)
REPS = 5
TORCH_REPS = 2
LATTICE = (128, 128, 64)
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
    """family -> ({column: engine call}, (graph build, loss maker) of the torch route or None) on fresh tensors of C = c."""
    L, m = f._L, int(pts.shape[0])
    rnd = lambda *shape: torch.from_numpy(rng.normal(0.0, 1.0, shape).astype(np.float32)).cuda()
    x, g, gm, gq = rnd(n, c), rnd(n, c), rnd(n, 4, c), rnd(m, c)
    outn, outm, outq = torch.empty((n, c), dtype=torch.float32, device="cuda"), torch.empty((n, 4, c), dtype=torch.float32, device="cuda"), \
        torch.empty((m, c), dtype=torch.float32, device="cuda")
    gradn, gradq = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((m, 3), dtype=torch.float32, device="cuda")
    POLY6 = pkg.SPH_AGGREGATE_WEIGHT_POLY6
    plain = pkg.aggregate_config(radius=h, channels=c, weight=POLY6)
    mom = pkg.aggregate_config(radius=h, channels=c, weight=POLY6, flags=pkg.SPH_AGGREGATE_MOMENTS)
    pos = f.positions(device=True)
    R2 = float(np.float32(h) * np.float32(h))
    p = lambda t: vp(t.data_ptr())

    def loss(recv, send, targets, rows, up):
        def run():
            P = pos.clone().requires_grad_(True)
            T = P if targets is None else targets[:, :3].clone().requires_grad_(True)
            d = P[send] - T[recv]
            w = (R2 - (d * d).sum(dim=1)) ** 3
            out = torch.zeros((rows, c), dtype=torch.float32, device="cuda").index_add_(0, recv, w[:, None] * x[send])
            (out * up).sum().backward()
            return P.grad
        return run

    def torch_particles():
        recv, send = f.radius_graph(h)
        return loss(recv, send, None, n, g)

    def torch_query():
        off, idx = f.query_neighbors(pts, h, device=True)
        recv = torch.repeat_interleave(torch.arange(m, device="cuda"), off[1:] - off[:-1])
        return loss(recv, idx.to(torch.int64), pts, m, gq)

    def posgrad_query(want_points, want_particles):
        return lambda: call(f, L.sph_aggregate_posgrad_query, C.byref(plain), p(pts), m, p(x), p(gq), p(gradq) if want_points else None,
                            p(gradn) if want_particles else None)

    return {
        "particles": ({"posgrad": lambda: call(f, L.sph_aggregate_posgrad_particles, C.byref(plain), p(x), p(g), p(gradn)),
                       "forward": lambda: call(f, L.sph_aggregate_particles, C.byref(plain), p(x), p(outn), None),
                       "adjoint": lambda: call(f, L.sph_aggregate_adjoint_particles, C.byref(plain), p(g), p(outn))},
                      (lambda: f.radius_graph(h), torch_particles)),
        "moments": ({"posgrad": lambda: call(f, L.sph_aggregate_posgrad_particles, C.byref(mom), p(x), p(gm), p(gradn)),
                     "forward": lambda: call(f, L.sph_aggregate_particles, C.byref(mom), p(x), p(outm), None),
                     "adjoint": lambda: call(f, L.sph_aggregate_adjoint_particles, C.byref(mom), p(gm), p(outn))}, None),
        "query": ({"posgrad": posgrad_query(True, True), "posgrad_points": posgrad_query(True, False), "posgrad_particles": posgrad_query(False, True),
                   "forward": lambda: call(f, L.sph_aggregate_query, C.byref(plain), p(pts), m, p(x), p(outq), None),
                   "adjoint": lambda: call(f, L.sph_aggregate_adjoint_query, C.byref(plain), p(pts), m, p(gq), p(outn))},
                  (lambda: f.query_neighbors(pts, h, device=True), torch_query)),
    }


def torch_columns(stream, graph, make):
    import torch
    res = {}
    try:
        with torch.cuda.stream(stream):
            res["graph"] = timing.events(graph, stream, reps=TORCH_REPS, warm=1)
            res["loss"] = timing.events(make(), stream, reps=TORCH_REPS, warm=1)
    except RuntimeError as err:
        res["not_measured"] = str(err).splitlines()[0][:200]
    torch.cuda.empty_cache()
    return res


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path([a for a in sys.argv[1:] if not a.startswith("--")], "posgrad")
    cfg3, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    n, h = len(rec), float(sp.param_h)
    rng = np.random.default_rng(1)
    with torch.cuda.stream(stream):
        pts = lattice_points(f, torch, np)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    res = timing.header("tools/time_posgrad.py", cfg3, rec, reps=REPS, torch_reps=TORCH_REPS, radius="h", weight="poly6", query_points=int(pts.shape[0]), regimes={})
    for label, substep, state in timing.regimes(f, download=False):
        r = {}
        for c in CHANNELS:
            with torch.cuda.stream(stream):
                todo = cases(f, torch, rng, np, n, pts, h, c)
            stream.synchronize()
            for name, (calls, route) in todo.items():
                v = {}
                for column, fn in calls.items():
                    t, grid_us = series(f, fn, reps=REPS, warm=2)
                    v[column] = t
                    if column == "posgrad":
                        v["grid_build"] = grid_us
                v["posgrad_over_forward"] = v["posgrad"]["median_us"] / v["forward"]["median_us"]
                v["posgrad_over_adjoint"] = v["posgrad"]["median_us"] / v["adjoint"]["median_us"]
                if route is not None and c in TORCH_CHANNELS:
                    v["torch"] = torch_columns(stream, *route)
                r.setdefault(name, {})[str(c)] = v
                print(label, name, "C", c, json.dumps({k: round(t["median_us"]) for k, t in v.items() if isinstance(t, dict) and "median_us" in t}), "torch",
                      json.dumps({k: (round(t["median_us"]) if isinstance(t, dict) else t) for k, t in v.get("torch", {}).items()}), flush=True)
            del todo
            torch.cuda.empty_cache()
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
