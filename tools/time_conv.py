"""Timing of the filter-grid basis sums and continuous_conv (include/sph_abi.h "filter-grid basis sums") at config 3
(4 M particles, 128^3 cells, h = cellSize) after 1 substep and after 300 substeps (the compressed regime), R = h,
K = 4 (B = 64 planes), Cin = Cout = 16, 32, 64, particle targets with SELF and the poly6 weight, all in ONE process on ONE state.  Per
regime and channel count:

  basis            sph_aggregate_basis_particles into a preallocated (n, 64, C) tensor: the engine's own brackets (SPH_OPT_TIMING, class
                   `other`: ids, stage, walk); `store_GBps` is n * 64 * C * 4 bytes over the median, the rate at which the output alone
                   is written
  adjoint          sph_aggregate_basis_adjoint_particles of that tensor, the same brackets
  gemm             A.reshape(n, 64 C) @ filters.reshape(64 C, C) in torch, between device events
  conv_forward     SPHFluidGPU.continuous_conv end to end (check_state=False) at max_basis_bytes = 2^31 (the default: blocks of two input
                   channels here) and at 2^37 (one block), between device events
  conv_forward_backward   the same with y.sum().backward() for x and filters (the basis sums are recomputed in the backward)
  sum, sum_moments sph_aggregate_particles SUM and SUM with MOMENTS at the same C: the floor of the walk and the 4-plane relative
  torch            the route without the engine's kernel, where it fits in memory: radius_graph (`graph`), the trilinear coefficients per
                   edge (`coefficients`), eight index_add_ into (n * 64, C) (`reduce`); the own slot is not in the list.  In the compressed
                   regime at C = 16 only, one run.  A route that does not fit is `not_measured`.
No ratio is fixed in advance.

  python tools/time_conv.py [out.json] [--trace CSV]
  python tools/time_conv.py --trace-run       a short run for `rocprofv3 --kernel-trace --stats --output-format csv`: C = 16, the compressed
                                              regime, three calls of the basis sums and of the adjoint; --trace CSV adds the per-kernel
                                              averages to the result as `kernel_trace`
Without an argument the result goes to time_conv.json in the current directory; profiles/r32_time_conv.json is the committed record of
the kernels in the tree.
"""
from __future__ import annotations

import csv
import ctypes as C
import json
import sys

import timing
from timing import pkg, series

CHANNELS = (16, 32, 64)
K = 4
B = K ** 3
REPS = 5
TORCH_REPS = 2
KERNELS = ("k_aggregate_basis", "k_aggregate_stage", "k_aggregate<", "k_neighbors_ids")
vp = C.c_void_p


def call(f, fn, *args):
    info = pkg.SphAggregateInfo()
    pkg.engine._check(fn(f._h, *args, C.byref(info)))


def torch_route(f, torch, x, h, c, n):
    """(graph, coefficients, reduce): the three phases as closures; each returns what the next needs."""
    half = 0.5 * (K - 1)

    def graph():
        return f.radius_graph(h)

    def coefficients(recv, send, pos):
        d = pos[send] - pos[recv]
        w = (h * h - (d * d).sum(dim=1)) ** 3
        g = (d / h + 1.0) * half
        i = g.floor().clamp_(0, K - 2)
        fr = g - i
        return i.to(torch.int64), fr, w

    def reduce(recv, send, i, fr, w):
        out = torch.zeros((n * B, c), dtype=torch.float32, device="cuda")
        xs = x[send]
        for corner in range(8):
            cx, cy, cz = corner & 1, (corner >> 1) & 1, corner >> 2
            b = ((i[:, 2] + cz) * K + (i[:, 1] + cy)) * K + (i[:, 0] + cx)
            coef = w * (fr[:, 0] if cx else 1.0 - fr[:, 0]) * (fr[:, 1] if cy else 1.0 - fr[:, 1]) * (fr[:, 2] if cz else 1.0 - fr[:, 2])
            out.index_add_(0, recv * B + b, coef[:, None] * xs)
        return out

    return graph, coefficients, reduce


def torch_columns(f, torch, np, stream, x, h, c, n, reps):
    res = {}
    try:
        with torch.cuda.stream(stream):
            graph, coefficients, reduce = torch_route(f, torch, x, h, c, n)
            pos = torch.from_numpy(np.ascontiguousarray(f.download()["pos"][:, :3])).cuda()
            warm = 1 if reps > 1 else 0
            res["graph"] = timing.events(graph, stream, reps=reps, warm=warm)
            recv, send = graph()
            res["edges"] = int(recv.shape[0])
            res["coefficients"] = timing.events(lambda: coefficients(recv, send, pos), stream, reps=reps, warm=warm)
            i, fr, w = coefficients(recv, send, pos)
            res["reduce"] = timing.events(lambda: reduce(recv, send, i, fr, w), stream, reps=reps, warm=warm)
            del recv, send, i, fr, w
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
    out_path = timing.out_path(plain, "conv")
    cfg3, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    n, h = len(rec), float(sp.param_h)
    L = f._L
    gen = torch.Generator().manual_seed(1)

    def tensors(c):
        with torch.cuda.stream(stream):
            x = torch.randn((n, c), generator=gen).cuda()
            filt = (torch.randn((K, K, K, c, c), generator=gen) / B).cuda()
            A = torch.empty((n, B, c), dtype=torch.float32, device="cuda")
            outn = torch.empty((n, c), dtype=torch.float32, device="cuda")
        stream.synchronize()
        return x, filt, A, outn

    def basis_calls(c, x, A, outn):
        bc = pkg.basis_config(radius=h, channels=c, size=K, flags=pkg.SPH_AGGREGATE_SELF)
        return (lambda: call(f, L.sph_aggregate_basis_particles, C.byref(bc), vp(x.data_ptr()), vp(A.data_ptr()), None),
                lambda: call(f, L.sph_aggregate_basis_adjoint_particles, C.byref(bc), vp(A.data_ptr()), vp(outn.data_ptr())))

    if trace_run:
        f.DispatchN(300)
        f.sync()
        x, filt, A, outn = tensors(16)
        for fn in basis_calls(16, x, A, outn):
            for _ in range(3):
                fn()
            f.sync()
        f.close()
        return
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    res = timing.header("tools/time_conv.py", cfg3, rec, reps=REPS, torch_reps=TORCH_REPS, radius="h", size=K, planes=B, weight="poly6", self_=True, regimes={})
    for label, substep, state in timing.regimes(f, download=False):
        r = {}
        for c in CHANNELS:
            x, filt, A, outn = tensors(c)
            forward, adjoint = basis_calls(c, x, A, outn)
            v = {"out_bytes": n * B * c * 4}
            v["basis"], v["grid_build"] = series(f, forward, reps=REPS, warm=1)
            v["basis"]["store_GBps"] = v["out_bytes"] / v["basis"]["median_us"] / 1000.0
            v["adjoint"] = series(f, adjoint, reps=REPS, warm=1)[0]
            with torch.cuda.stream(stream):
                v["gemm"] = timing.events(lambda: A.reshape(n, B * c) @ filt.reshape(B * c, c), stream, reps=REPS, warm=1)
            del A
            torch.cuda.empty_cache()
            plane = torch.empty((n, 4, c), dtype=torch.float32, device="cuda")
            for name, flags in (("sum", pkg.SPH_AGGREGATE_SELF), ("sum_moments", pkg.SPH_AGGREGATE_SELF | pkg.SPH_AGGREGATE_MOMENTS)):
                ac = pkg.aggregate_config(radius=h, channels=c, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6, flags=flags)
                v[name] = series(f, lambda: call(f, L.sph_aggregate_particles, C.byref(ac), vp(x.data_ptr()), vp(plane.data_ptr()), None), reps=REPS, warm=1)[0]
            del plane
            for tag, limit in (("2^31", 2 ** 31), ("2^37", 2 ** 37)):
                def both():
                    xg, fg = x.detach().requires_grad_(True), filt.detach().requires_grad_(True)
                    f.continuous_conv(xg, fg, h, check_state=False, max_basis_bytes=limit).sum().backward()

                for name, fn in (("conv_forward_", lambda: f.continuous_conv(x, filt, h, check_state=False, max_basis_bytes=limit)), ("conv_forward_backward_", both)):
                    try:
                        with torch.cuda.stream(stream):
                            v[name + tag] = timing.events(fn, stream, reps=3, warm=1)
                    except RuntimeError as err:                                         # (one block of 64 channels is 69 GB, three times over in the backward)
                        v[name + tag] = {"not_measured": str(err).splitlines()[0][:200]}
                    torch.cuda.empty_cache()
            if label != "compressed":
                v["torch"] = torch_columns(f, torch, np, stream, x, h, c, n, TORCH_REPS)
            elif c == CHANNELS[0]:
                v["torch"] = torch_columns(f, torch, np, stream, x, h, c, n, 1)
            r[str(c)] = v
            print(label, "C", c, json.dumps({k: (round(t["median_us"]) if isinstance(t, dict) and "median_us" in t else None) for k, t in v.items() if isinstance(t, dict)}),
                  "store GB/s", round(v["basis"]["store_GBps"]), flush=True)
            del x, filt, outn
            torch.cuda.empty_cache()
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    if trace:
        res["kernel_trace"] = dict(read_trace(trace), note="rocprofv3 --kernel-trace --stats of --trace-run: C = 16, compressed regime, averages per launch")
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
