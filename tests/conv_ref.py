"""Restatement of the filter-grid basis sums and their adjoint (include/sph_abi.h "filter-grid basis sums") in numpy
float32, operation by operation and independent of the C++ twin: the accepted candidates of every row and their order come from
aggregate_ref.edges (pkg.neighbors_host lists), the per-axis coordinates, the 8 corners and their coefficients are computed here, and
every accumulator takes its terms sequentially with one rounding per product and per sum.  Also the float64 pieces the bounds of the
tests are made of, and the cases the CPU and the GPU tests share."""
import numpy as np

import aggregate_ref as AR
import neighbors_ref as NR

F = np.float32
U = 2.0 ** -24


def axis(d, radius, K):
    """(i, lo, hi) of one axis: u = d / R, g = (u + 1) * half, i = (int)g clamped to [0, K - 2], f = g - i, lo = 1 - f, hi = f."""
    half = F(F(0.5) * F(K - 1))
    u = (np.asarray(d, F) / F(radius)).astype(F)
    g = ((u + F(1.0)).astype(F) * half).astype(F)
    i = np.clip(g.astype(np.int64), 0, K - 2)                   # (the conversion truncates; g >= 0 for an accepted candidate)
    f = (g - i.astype(F)).astype(F)
    return i, (F(1.0) - f).astype(F), f


def corners(d, w, radius, K):
    """(b int64 (E, 8), coef float32 (E, 8)) in ascending plane b: corner t has cx = t & 1, cy = (t >> 1) & 1, cz = t >> 2."""
    ix, lx, hx = axis(d[:, 0], radius, K)
    iy, ly, hy = axis(d[:, 1], radius, K)
    iz, lz, hz = axis(d[:, 2], radius, K)
    b = np.zeros((len(d), 8), np.int64)
    coef = np.zeros((len(d), 8), F)
    for t in range(8):
        cx, cy, cz = t & 1, (t >> 1) & 1, t >> 2
        b[:, t] = ((iz + cz) * K + (iy + cy)) * K + (ix + cx)
        wx, wy, wz = (hx if cx else lx), (hy if cy else ly), (hz if cz else lz)
        coef[:, t] = (w * ((wx * wy).astype(F) * wz).astype(F)).astype(F)
    return b, coef


def terms(pkg, rec, sp, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False):
    """The accepted pairs in the engine's order with their planes and coefficients: (rows, recv, send, b, coef, w)."""
    rows, recv, send, d, r2 = AR.edges(pkg, rec, sp, radius, points, self_, fluid_only)
    w = AR.weights(weight, radius, r2)
    b, coef = corners(d, w, radius, size)
    assert len(b) == 0 or (b.min() >= 0 and b.max() < size ** 3 and (np.diff(b, axis=1) > 0).all())
    return rows, recv, send, b, coef, w


def _ranks(group):
    """For edges listed group by group (group ids non-decreasing): the edges of rank t of every group, t = 0, 1, ..."""
    cnt = np.bincount(group, minlength=1) if len(group) else np.zeros(1, np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])
    rank = np.arange(len(group)) - first[group]
    by_rank = np.argsort(rank, kind="stable")
    longest = int(cnt.max()) if len(group) else 0
    starts = np.searchsorted(rank[by_rank], np.arange(longest + 1), side="left")
    return [by_rank[starts[t]:starts[t + 1]] for t in range(longest)]


def basis(pkg, rec, sp, x, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False):
    """(out float32 (rows, K^3, C), counts uint32 (rows,))."""
    x = np.ascontiguousarray(x, F).reshape(len(rec), -1)
    rows, recv, send, b, coef, w = terms(pkg, rec, sp, radius, points, size, weight, self_, fluid_only)
    acc = np.zeros((rows, size ** 3, x.shape[1]), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in _ranks(recv):                                  # the t-th accepted candidate of every row that has one
            r = recv[e]
            for t in range(8):                                  # (8 distinct planes: their order does not enter the bytes)
                acc[r, b[e, t]] = (acc[r, b[e, t]] + (coef[e, t][:, None] * x[send[e]]).astype(F)).astype(F)
    return acc, np.bincount(recv, minlength=rows).astype(np.uint32)


def adjoint_order(pkg, rec, sp, recv, send, points=None):
    """The permutation of the edges into the adjoint's order: by particle, then by the row's (clamped cell, index): ascending sorted
    slot for particle targets, ascending (cell of the point, point index) for query targets."""
    cell = NR.cells(pkg, rec["pos"] if points is None else points, sp)
    return np.lexsort((recv, cell[recv], send))


def basis_adjoint(pkg, rec, sp, h, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False):
    """out float32 (n, C): per particle the rows in the adjoint's order, per row the 8 corners in ascending b, acc = acc + coef * h."""
    rows, recv, send, b, coef, w = terms(pkg, rec, sp, radius, points, size, weight, self_, fluid_only)
    h = np.ascontiguousarray(h, F).reshape(rows, size ** 3, -1)
    order = adjoint_order(pkg, rec, sp, recv, send, points)
    recv, send, b, coef = recv[order], send[order], b[order], coef[order]
    acc = np.zeros((len(rec), h.shape[2]), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in _ranks(send):
            k = send[e]
            for t in range(8):
                acc[k] = (acc[k] + (coef[e, t][:, None] * h[recv[e], b[e, t]]).astype(F)).astype(F)
    return acc


def dense(pkg, rec, sp, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False):
    """The operator as float64 (rows, K^3, n) of the fp32 coefficients."""
    rows, recv, send, b, coef, w = terms(pkg, rec, sp, radius, points, size, weight, self_, fluid_only)
    T = np.zeros((rows, size ** 3, len(rec)))
    for t in range(8):
        np.add.at(T, (recv, b[:, t], send), coef[:, t].astype(np.float64))
    return T


def gamma(k):
    return AR.gamma(np.asarray(k, np.float64))


# (size K, weight, self_, radius in h, C): every K, both weights, SELF on and off, the three stencils (R = 0.7 h and h: one cell;
# 2 h, 2.5 h: two and three), odd channel counts
PARTICLE_CASES = [
    (2, "one", False, 1.0, 1),
    (3, "poly6", True, 2.0, 3),
    (4, "poly6", False, 1.0, 5),
    (4, "one", True, 2.5, 2),
    (3, "one", False, 0.7, 4),
    (2, "poly6", True, 3.0, 3),
]
QUERY_CASES = [(K, w, False, fac, c) for K, w, s, fac, c in PARTICLE_CASES[:5]]


def planes_for(rows, size, c, seed=71):
    return np.random.default_rng(seed + c + size).normal(0.0, 1.0, (rows, size ** 3, c)).astype(F)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1)) if len(got) else []
    assert got.tobytes() == want.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"
