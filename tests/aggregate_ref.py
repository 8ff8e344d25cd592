"""Restatement of the fused neighbourhood reductions (include/sph_abi.h "fused neighbourhood reductions") in numpy,
independent of the C++ twin: the candidate order of every row comes from pkg.neighbors_host (CSR, SELF as asked), d and r2 are
recomputed with scalar_ref.dot3 / fma32, every channel is accumulated sequentially in np.float32 (one rounding per product and per sum,
no fused multiply-add), and extrema are taken through the ordered-bits key.  Also the cases, values and comparison that the CPU and the
GPU tests share."""
import numpy as np

import scalar_ref as SR

F = np.float32
U = np.uint32
LOWEST, HIGHEST = U(0x007FFFFF), U(0xFF800000)                 # ordered(-inf), ordered(+inf)


def ordered(v):
    """float32 bits -> uint32 keys in numeric order (-0 below +0)."""
    u = np.ascontiguousarray(v, F).view(U)
    return np.where(u & U(0x80000000), ~u, u | U(0x80000000)).astype(U)


def unordered(o):
    o = np.ascontiguousarray(o, U)
    return np.where(o & U(0x80000000), o & U(0x7FFFFFFF), ~o).astype(U).view(F)


def edges(pkg, rec, sp, radius, points=None, self_=False, fluid_only=False):
    """The accepted candidates of every row in the engine's order: (rows, recv, send, d (E, 3) float32, r2 (E,) float32)."""
    off, idx = pkg.neighbors_host(rec, sp, radius, points=points, self_=self_ and points is None)
    rows = len(off) - 1
    recv = np.repeat(np.arange(rows, dtype=np.int64), np.diff(off))
    send = idx.astype(np.int64)
    pos = rec["pos"][:, :3].astype(F)
    tgt = pos if points is None else np.asarray(points, F)[:, :3]
    own = (send == recv) if points is None else np.zeros(len(send), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (pos[send] - tgt[recv]).astype(F)
        d[own] = F(0)
        r2 = SR.dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]).astype(F)
    r2[own] = F(0)
    R2 = F(radius) * F(radius)
    assert (r2[~own] < R2).all(), "the lists hold a candidate this restatement rejects"
    if fluid_only:
        ghost = rec["isGhost"] != 0
        keep = ~ghost[send]
        if points is None:
            keep &= ~ghost[recv]
        recv, send, d, r2 = recv[keep], send[keep], d[keep], r2[keep]
    return rows, recv, send, d, r2


def weights(weight, radius, r2):
    if weight == "one":
        return np.ones(len(r2), F)
    R2 = F(radius) * F(radius)
    t = (R2 - r2).astype(F)
    return ((t * t).astype(F) * t).astype(F)


def aggregate(pkg, rec, sp, values, radius, points=None, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False):
    """(out float32 (rows, C) or (rows, 4, C), counts uint32 (rows,))."""
    x = np.ascontiguousarray(values, F).reshape(len(rec), -1)
    C = x.shape[1]
    rows, recv, send, d, r2 = edges(pkg, rec, sp, radius, points, self_, fluid_only)
    cnt = np.bincount(recv, minlength=rows).astype(U)
    with np.errstate(invalid="ignore", over="ignore"):
        val = x[send] if not delta else (x[send] - x[recv]).astype(F)
        if op in ("max", "min"):
            key = ordered(val)
            nan = np.isnan(val)
            if op == "max":
                best = np.full((rows, C), LOWEST, U)
                np.maximum.at(best, recv, np.where(nan, LOWEST, key))
            else:
                best = np.full((rows, C), HIGHEST, U)
                np.minimum.at(best, recv, np.where(nan, HIGHEST, key))
            return unordered(best).reshape(rows, C), cnt
        w = weights(weight, radius, r2)
        planes = 4 if moments else 1
        acc = np.zeros((planes, rows, C), F)
        W = np.zeros(rows, F)
        first = np.zeros(rows + 1, np.int64)
        np.cumsum(cnt, out=first[1:])
        rank = np.arange(len(recv)) - first[recv]
        by_rank = np.argsort(rank, kind="stable")
        longest = int(cnt.max()) if rows else 0
        starts = np.searchsorted(rank[by_rank], np.arange(longest + 1), side="left")
        for t in range(longest):                                # the t-th accepted candidate of every row that has one
            e = by_rank[starts[t]:starts[t + 1]]
            r = recv[e]
            we = w[e][:, None]
            acc[0, r] = (acc[0, r] + (we * val[e]).astype(F)).astype(F)
            W[r] = (W[r] + w[e]).astype(F)
            for a in range(planes - 1):
                wd = (w[e] * d[e, a]).astype(F)[:, None]
                acc[1 + a, r] = (acc[1 + a, r] + (wd * val[e]).astype(F)).astype(F)
        if op == "mean":
            ok = W != 0
            acc[0] = np.where(ok[:, None], (acc[0] / np.where(ok, W, F(1))[:, None]).astype(F), F(0))
    out = np.ascontiguousarray(np.moveaxis(acc, 0, 1)) if moments else acc[0]
    return out, cnt


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


# (op, weight, self_, delta, moments, radius in h, C): every op, both weights, SELF / DELTA / MOMENTS where legal, the three stencils and
# the channel counts 1, 3, 4, 5, 17, 128 (odd widths, a seam of every chunk width, the cap), pairwise rather than as a full product
PARTICLE_CASES = [
    ("sum", "one", False, False, False, 1.0, 1),
    ("sum", "poly6", True, False, True, 2.0, 3),
    ("sum", "one", False, True, True, 1.0, 17),
    ("sum", "poly6", False, True, False, 3.0, 4),
    ("sum", "one", True, True, True, 3.0, 128),
    ("mean", "one", True, True, False, 2.0, 5),
    ("mean", "poly6", False, False, False, 1.0, 128),
    ("mean", "poly6", True, False, False, 3.0, 17),
    ("max", "one", False, False, False, 3.0, 5),
    ("max", "one", True, True, False, 1.0, 17),
    ("min", "one", False, True, False, 2.0, 4),
    ("min", "one", True, False, False, 1.0, 1),
    ("min", "one", False, False, False, 2.0, 128),
]
QUERY_CASES = [(op, w, False, False, mom, fac, c) for op, w, s, d, mom, fac, c in PARTICLE_CASES if not (s or d)] + [
    ("sum", "poly6", False, False, True, 2.0, 3), ("sum", "one", False, False, True, 3.0, 17), ("mean", "one", False, False, False, 2.0, 5),
    ("max", "one", False, False, False, 1.0, 4)]


def values_for(n, c, seed=5):
    return np.random.default_rng(seed + c).normal(0.0, 1.0, (n, c)).astype(F)


def radius_of(sp, fac):
    return float(F(fac) * F(sp.param_h))


def same_bytes(got, want, what):
    (g_out, g_cnt), (w_out, w_cnt) = got, want
    assert g_out.dtype == F and g_cnt.dtype == np.uint32 and g_out.shape == w_out.shape and g_cnt.shape == w_cnt.shape, what
    assert g_cnt.tobytes() == w_cnt.tobytes(), f"{what}: counts differ"
    bad = np.flatnonzero((g_out.view(np.uint32) != w_out.view(np.uint32)).reshape(len(g_out), -1).any(axis=1))
    assert g_out.tobytes() == w_out.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"
