"""Timing of the position gradients of the basis sums (include/sph_abi.h "position gradients of the basis sums") at
config 3 (4 M particles, 128^3 cells, h = cellSize) after 1 substep and after 300 substeps (the compressed regime),
R = h, K = 4 (B = 64 planes), the poly6 weight, C = 16, 32, 64, all in ONE process on ONE state.  Per regime and channel count:

  particles      sph_aggregate_basis_posgrad_particles | the basis forward sph_aggregate_basis_particles | the basis adjoint
                 sph_aggregate_basis_adjoint_particles | sph_aggregate_posgrad_particles with MOMENTS of the same C (`moments`)
  query          sph_aggregate_basis_posgrad_query with both outputs from a lattice of 128 x 128 x 64 points across the grid's box | with
                 the points' output alone | with the particles' output alone | sph_aggregate_basis_query | sph_aggregate_basis_adjoint_query
  conv           SPHFluidGPU.continuous_conv forward + backward (Cin = Cout = C, SELF, check_state=False, max_basis_bytes 2^31) without
                 and with positions=, between device events
  torch          the route without the engine's kernel, C = 16 only, one run: radius_graph (`graph`), then from a positions tensor that
                 requires grad the trilinear coefficients per edge, eight index_add_ into (n * 64, C) and backward() of sum(A * g) (`loss`);
                 a route that does not fit is `not_measured`
The engine's columns are its own brackets (SPH_OPT_TIMING, class `other`: ids, binning, stage, walks).  g is filled on the device.  No
ratio is fixed in advance.

  python tools/time_conv_posgrad.py [out.json]
Without an argument the result goes to time_conv_posgrad.json in the current directory; profiles/r34_time_conv_posgrad.json is the
committed record of the kernels in the tree.
"""
from __future__ import annotations

import ctypes as C
import json
import sys

import timing
from timing import pkg, series
from time_posgrad import lattice_points

CHANNELS = (16, 32, 64)
TORCH_CHANNELS = (16,)
K = 4
B = K ** 3
REPS = 3
vp = C.c_void_p


def call(f, fn, *args):
    info = pkg.SphAggregateInfo()
    pkg.engine._check(fn(f._h, *args, C.byref(info)))


def torch_loss(f, torch, pos, x, g, h, n, c):
    """(graph, loss maker): the list, then coefficients from a positions leaf, index_add_ and backward()."""
    half = 0.5 * (K - 1)

    def make():
        recv, send = f.radius_graph(h)

        def run():
            P = pos.clone().requires_grad_(True)
            d = P[send] - P[recv]
            w = (h * h - (d * d).sum(dim=1)) ** 3
            gr = (d / h + 1.0) * half
            i = gr.detach().floor().clamp_(0, K - 2)
            fr = gr - i
            i = i.to(torch.int64)
            out = torch.zeros((n * B, c), dtype=torch.float32, device="cuda")
            xs = x[send]
            for corner in range(8):
                cx, cy, cz = corner & 1, (corner >> 1) & 1, corner >> 2
                b = ((i[:, 2] + cz) * K + (i[:, 1] + cy)) * K + (i[:, 0] + cx)
                coef = w * (fr[:, 0] if cx else 1.0 - fr[:, 0]) * (fr[:, 1] if cy else 1.0 - fr[:, 1]) * (fr[:, 2] if cz else 1.0 - fr[:, 2])
                out = out.index_add(0, recv * B + b, coef[:, None] * xs)
            (out * g.reshape(n * B, c)).sum().backward()
            return P.grad
        return run
    return (lambda: f.radius_graph(h)), make


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path([a for a in sys.argv[1:] if not a.startswith("--")], "conv_posgrad")
    cfg3, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    n, h = len(rec), float(sp.param_h)
    L = f._L
    with torch.cuda.stream(stream):
        pts = lattice_points(f, torch, np)
    m = int(pts.shape[0])
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    res = timing.header("tools/time_conv_posgrad.py", cfg3, rec, reps=REPS, radius="h", size=K, planes=B, weight="poly6", query_points=m, regimes={})
    p = lambda t: vp(t.data_ptr())
    POLY6 = pkg.SPH_AGGREGATE_WEIGHT_POLY6
    for label, substep, state in timing.regimes(f, download=False):
        r = {}
        for c in CHANNELS:
            with torch.cuda.stream(stream):
                torch.manual_seed(1 + c)
                x = torch.randn((n, c), dtype=torch.float32, device="cuda")
                g = torch.randn((n, B, c), dtype=torch.float32, device="cuda")
                gq = torch.randn((m, B, c), dtype=torch.float32, device="cuda")
                gm = torch.randn((n, 4, c), dtype=torch.float32, device="cuda")
                outn = torch.empty((n, c), dtype=torch.float32, device="cuda")
                gradn, gradq = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((m, 3), dtype=torch.float32, device="cuda")
            stream.synchronize()
            bc = pkg.basis_config(radius=h, channels=c, size=K)
            mom = pkg.aggregate_config(radius=h, channels=c, weight=POLY6, flags=pkg.SPH_AGGREGATE_MOMENTS)

            def query(want_points, want_particles):
                return lambda: call(f, L.sph_aggregate_basis_posgrad_query, C.byref(bc), p(pts), m, p(x), p(gq), p(gradq) if want_points else None,
                                    p(gradn) if want_particles else None)

            # (the forwards write over g / gq: their contents do not matter to a timing, and a second tensor of that size is not needed)
            calls = {
                "particles": {"posgrad": lambda: call(f, L.sph_aggregate_basis_posgrad_particles, C.byref(bc), p(x), p(g), p(gradn)),
                              "adjoint": lambda: call(f, L.sph_aggregate_basis_adjoint_particles, C.byref(bc), p(g), p(outn)),
                              "moments": lambda: call(f, L.sph_aggregate_posgrad_particles, C.byref(mom), p(x), p(gm), p(gradn)),
                              "forward": lambda: call(f, L.sph_aggregate_basis_particles, C.byref(bc), p(x), p(g), None)},
                "query": {"posgrad": query(True, True), "posgrad_points": query(True, False), "posgrad_particles": query(False, True),
                          "adjoint": lambda: call(f, L.sph_aggregate_basis_adjoint_query, C.byref(bc), p(pts), m, p(gq), p(outn)),
                          "forward": lambda: call(f, L.sph_aggregate_basis_query, C.byref(bc), p(pts), m, p(x), p(gq), None)},
            }
            v = {}
            for name, columns in calls.items():
                t = {column: series(f, fn, reps=REPS, warm=1)[0] for column, fn in columns.items()}
                t["posgrad_over_forward"] = t["posgrad"]["median_us"] / t["forward"]["median_us"]
                t["posgrad_over_adjoint"] = t["posgrad"]["median_us"] / t["adjoint"]["median_us"]
                if "moments" in t:
                    t["posgrad_over_moments"] = t["posgrad"]["median_us"] / t["moments"]["median_us"]
                v[name] = t
            if c in TORCH_CHANNELS:
                tr = {}
                try:
                    with torch.cuda.stream(stream):
                        pos = f.positions(device=True)
                        graph, make = torch_loss(f, torch, pos, x, g, h, n, c)
                        tr["graph"] = timing.events(graph, stream, reps=1, warm=0)
                        tr["loss"] = timing.events(make(), stream, reps=1, warm=0)
                except RuntimeError as err:
                    tr["not_measured"] = str(err).splitlines()[0][:200]
                v["torch"] = tr
            del g, gq, gm
            torch.cuda.empty_cache()
            with torch.cuda.stream(stream):
                filt = torch.randn((K, K, K, c, c), dtype=torch.float32, device="cuda") / B
                pos = f.positions(device=True)

            def both(with_positions):
                def run():
                    xg, fg = x.detach().requires_grad_(True), filt.detach().requires_grad_(True)
                    pg = pos.detach().requires_grad_(True) if with_positions else None
                    f.continuous_conv(xg, fg, h, check_state=False, positions=pg).sum().backward()
                return run

            conv = {}
            for name, flag in (("forward_backward", False), ("forward_backward_positions", True)):
                try:
                    with torch.cuda.stream(stream):
                        conv[name] = timing.events(both(flag), stream, reps=REPS, warm=1)
                except RuntimeError as err:
                    conv[name] = {"not_measured": str(err).splitlines()[0][:200]}
                torch.cuda.empty_cache()
            v["conv"] = conv
            r[str(c)] = v
            brief = lambda t: {k: round(s["median_us"]) for k, s in t.items() if isinstance(s, dict) and "median_us" in s}
            print(label, "C", c, json.dumps({k: brief(t) for k, t in v.items()}), flush=True)
            del x, filt, outn
            torch.cuda.empty_cache()
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
