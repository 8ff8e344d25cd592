"""Brute-force restatement of the k nearest neighbours (include/sph_abi.h "k nearest neighbours"): all pairs in float64, the geometric
set |x_i - x_j|^2 < R^2 per row sorted by (distance, id) and cut at k.  It knows nothing of stencils, cells or fp32 keys, so it agrees
with the engine only where every particle lies inside the grid, and only on rows without a near tie: a row is a NEAR-TIE row when two
consecutive float64 distances among its first k + 1 accepted candidates differ by less than tol * R^2, or one of those distances lies
within tol * R^2 of R^2.  fp32 r2 is a few 2^-24 relative from the float64 value, so a wider gap cannot flip."""
import numpy as np

F = np.float32
TOL = 1e-6


def knn(pos, k, radius, points=None, self_=False, exclude=None, tol=TOL, chunk=256):
    """(idx (rows, k) int32 padded with -1, d2 (rows, k) float64 padded with +inf, counts (rows,) int64, near_tie (rows,) bool,
    edge (rows,) bool).  edge marks what the near-tie rows do not cover: a row with at most k accepted candidates and a REJECTED
    candidate within tol * R^2 of R^2, which fp32 may accept and so change the row's count; a test asserts that no row is one.
    pos: (n, >= 3) particle positions; points None: particle rows (the own particle left out unless self_); exclude: a bool mask of
    particles that are never candidates and whose own rows are empty."""
    X = np.asarray(pos, F)[:, :3].astype(np.float64)
    n = len(X)
    T = X if points is None else np.asarray(points, F)[:, :3].astype(np.float64)
    rows = len(T)
    R2 = float(F(radius)) ** 2
    out_idx = np.full((rows, k), -1, np.int32)
    out_d2 = np.full((rows, k), np.inf, np.float64)
    counts = np.zeros(rows, np.int64)
    near = np.zeros(rows, bool)
    edge = np.zeros(rows, bool)
    ids = np.arange(n)
    for a in range(0, rows, chunk):
        d = T[a:a + chunk, None, :] - X[None, :, :]
        with np.errstate(invalid="ignore"):
            r2 = (d * d).sum(axis=2)
        r2 = np.where(np.isnan(r2), np.inf, r2)
        if exclude is not None:
            r2[:, np.asarray(exclude, bool)] = np.inf
        if points is None:
            own = ids[None, :] == np.arange(a, a + r2.shape[0])[:, None]
            if not self_:
                r2 = np.where(own, np.inf, r2)
            if exclude is not None:
                r2[np.asarray(exclude, bool)[a:a + r2.shape[0]], :] = np.inf
        just_outside = ((r2 >= R2) & (r2 - R2 < tol * R2)).any(axis=1) if n else np.zeros(r2.shape[0], bool)
        edge[a:a + chunk] = just_outside & ((r2 < R2).sum(axis=1) <= k)
        r2 = np.where(r2 < R2, r2, np.inf)
        order = np.lexsort((np.broadcast_to(ids[None, :], r2.shape), r2), axis=1)[:, :k + 1] if n else np.zeros((r2.shape[0], 0), np.int64)
        sd = np.take_along_axis(r2, order, axis=1) if n else np.zeros((r2.shape[0], 0))
        ok = np.isfinite(sd)
        counts[a:a + chunk] = ok[:, :k].sum(axis=1)
        w = min(k, sd.shape[1])
        out_idx[a:a + chunk, :w] = np.where(ok[:, :w], order[:, :w], -1)
        out_d2[a:a + chunk, :w] = np.where(ok[:, :w], sd[:, :w], np.inf)
        if sd.shape[1] > 1:
            with np.errstate(invalid="ignore"):
                gap = np.diff(sd, axis=1)
            close = (gap < tol * R2) & ok[:, 1:]                                  # (inf - inf is NaN: not a gap between accepted candidates)
            near[a:a + chunk] = close.any(axis=1)
        near[a:a + chunk] |= ((R2 - sd < tol * R2) & ok).any(axis=1)
    return out_idx, out_d2, counts, near, edge
