"""Brute-force restatement of the neighbour lists (include/sph_abi.h "fixed-radius neighbour lists"): all pairs in float64, the geometric
set |x_i - x_j|^2 < R^2 per row, entries sorted by (cell index, particle id).  It knows nothing of stencils: it agrees with the engine
only where no pair sits on the sphere within rounding, which `margin` reports (the smallest |r^2 - R^2| / R^2 over all pairs)."""
import numpy as np

F = np.float32


def cells(pkg, pos, sp):
    """BuildGrid's cell index of every position, in fp32 as k_bin computes it: (x - gridMin) / cellSize, floor, clamp."""
    g = pkg.compute_grid_extents(sp)
    dims = np.array(list(g.dims), np.int64)
    gmin = np.array(list(g.gridMin), F)
    q = np.floor((np.asarray(pos, F)[:, :3] - gmin) / F(g.cellSize))
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, (dims - 1).astype(F))).astype(np.int64)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def inside_grid(pkg, pos, sp):
    """Every position strictly inside the grid's box?"""
    g = pkg.compute_grid_extents(sp)
    lo = np.array(list(g.gridMin), np.float64)
    hi = lo + np.array(list(g.dims), np.float64) * float(g.cellSize)
    p = np.asarray(pos, np.float64)[:, :3]
    return bool(((p > lo) & (p < hi)).all())


def brute_force(pkg, pos, sp, radius, points=None, self_=False, half=False, chunk=512):
    """(offsets int64[rows + 1], indices int32[total], margin).  pos: (n, >= 3) particle positions; points None: particle lists."""
    X = np.asarray(pos, F)[:, :3].astype(np.float64)
    n = len(X)
    T = X if points is None else np.asarray(points, F)[:, :3].astype(np.float64)
    R2 = float(F(radius)) ** 2
    perm = np.lexsort((np.arange(n), cells(pkg, pos, sp)))          # sorted slot -> id
    Xs = X[perm]
    counts = np.zeros(len(T), np.int64)
    parts = []
    margin = np.inf
    for a in range(0, len(T), chunk):
        d = T[a:a + chunk, None, :] - Xs[None, :, :]
        with np.errstate(invalid="ignore"):
            r2 = (d * d).sum(axis=2)
            mask = r2 < R2
            gap = np.abs(r2 - R2)
        ids = np.broadcast_to(perm[None, :], mask.shape)
        if points is None:
            rows = np.arange(a, a + mask.shape[0])[:, None]
            own = ids == rows
            gap = np.where(own, np.inf, gap)
            mask = np.where(own, bool(self_), mask & ((ids > rows) if half else True))
        if gap.size:
            margin = min(margin, float(np.nanmin(np.where(np.isnan(gap), np.inf, gap))) / R2)
        counts[a:a + chunk] = mask.sum(axis=1)
        parts.append(ids[mask])                                      # row-major: rows ascending, inside a row ascending sorted slot
    off = np.zeros(len(T) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    idx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return off, idx, margin


def rows_of(off, idx):
    return [idx[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def transpose_pairs(off, idx):
    """The set of (row, entry) pairs and of (entry, row) pairs as sorted int64 keys."""
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    n = np.int64(max(len(off) - 1, int(idx.max()) + 1 if len(idx) else 1))
    return np.sort(rows * n + idx), np.sort(idx.astype(np.int64) * n + rows)
