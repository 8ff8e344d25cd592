"""Brute-force float64 restatement of the free-surface shell (include/sph_abi.h "free-surface particles"): all pairs from the fp32
positions, no grid, no cells -- only the pairs further apart along x than R are not formed (rows and candidates are taken in the order
of x, a chunk of rows against the window of candidates within R of the chunk's x range).  Pass 1 gives per row count, W = sum w,
S = sum w d (w = (R^2 - r^2)^2, d = x_j - x), the sums that bound the fp32 twin's rounding, and from them offsetRatio, normal and the
shell flag; pass 2 the crest sum over the reference's own shell.  It knows nothing of stencils, so it agrees with the engine only
where every particle lies inside the grid."""
import numpy as np

F = np.float32
U = 2.0 ** -24                                        # unit roundoff of fp32
EDGE = 8.0 * U                                        # |R^2 - r^2| <= EDGE * R^2: fp32 may decide the candidate the other way


def _windows(Xc, Tr, R, chunk):
    """Chunks of rows in ascending x with the candidates that can be within R of them: (rows of the chunk, candidates of the window)."""
    co = np.argsort(Xc[:, 0], kind="stable")
    ro = np.argsort(Tr[:, 0], kind="stable")
    cx = Xc[co, 0]
    for a in range(0, len(ro), chunk):
        r = ro[a:a + chunk]
        lo, hi = np.searchsorted(cx, Tr[r[0], 0] - R, "left"), np.searchsorted(cx, Tr[r[-1], 0] + R, "right")
        yield r, co[lo:hi]


def shell(pos, radius, offset=0.10, min_count=0, points=None, exclude=None, chunk=256):
    """A dict of per-row arrays: count, W, S (rows, 3), boundS (rows, 3) = sum_j R^2 t_j |d_jk|, boundW = sum_j R^2 t_j, flipS / flipW
    (what candidates on the sphere within rounding can add), edge (the row has such a candidate), ratio, normal, member, isolated, crest.
    pos: (n, >= 3) particle positions; points None: particle rows (the own particle left out); exclude: a bool mask of particles that are
    never candidates and whose own rows are all zero.  Non-finite positions are candidates of nobody and have all-zero rows."""
    X = np.asarray(pos, F)[:, :3].astype(np.float64)
    n = len(X)
    T = X if points is None else np.asarray(points, F)[:, :3].astype(np.float64)
    rows = len(T)
    R = float(F(radius))
    R2 = R * R
    ex = np.zeros(n, bool) if exclude is None else np.asarray(exclude, bool)
    out = dict(count=np.zeros(rows, np.int64), W=np.zeros(rows), S=np.zeros((rows, 3)), boundS=np.zeros((rows, 3)), boundW=np.zeros(rows),
               flipS=np.zeros((rows, 3)), flipW=np.zeros(rows), edge=np.zeros(rows, bool))
    cand = np.flatnonzero(np.isfinite(X).all(axis=1) & ~ex)
    walks = np.isfinite(T).all(axis=1)
    if points is None:
        walks &= ~ex
    tr = np.flatnonzero(walks)
    for r, c in _windows(X[cand], T[tr], R, chunk):
        r, c = tr[r], cand[c]
        d = [X[c, k][None, :] - T[r, k][:, None] for k in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if points is None:
            r2[r[:, None] == c[None, :]] = np.inf
        acc = r2 < R2
        t = np.where(acc, R2 - r2, 0.0)
        w = t * t
        near = np.abs(R2 - r2) <= EDGE * R2
        flip = np.where(near, (2.0 * EDGE * R2) ** 2, 0.0)
        out["count"][r] = acc.sum(axis=1)
        out["W"][r] = w.sum(axis=1)
        out["boundW"][r] = R2 * t.sum(axis=1)
        out["edge"][r] = near.any(axis=1)
        out["flipW"][r] = flip.sum(axis=1)
        for k in range(3):
            out["S"][r, k] = (w * d[k]).sum(axis=1)
            out["boundS"][r, k] = R2 * (t * np.abs(d[k])).sum(axis=1)
            out["flipS"][r, k] = (flip * np.abs(d[k])).sum(axis=1)
    s = np.sqrt((out["S"] ** 2).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["ratio"] = np.where(out["W"] > 0, s / (R * out["W"]), 0.0)
        out["normal"] = np.where(s[:, None] > 0, -out["S"] / s[:, None], 0.0)
    out["isolated"] = (out["count"] == 0) & walks
    out["member"] = walks & ((out["count"] == 0) | (out["count"] < min_count) | (s > offset * R * out["W"]))
    out["crest"] = np.zeros(rows)
    if points is None:
        m = np.flatnonzero(out["member"])
        N = out["normal"]
        for r, c in _windows(X[m], X[m], R, chunk):
            r, c = m[r], m[c]
            d = [X[c, k][None, :] - X[r, k][:, None] for k in range(3)]
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            r2[r[:, None] == c[None, :]] = np.inf
            behind = (r2 < R2) & (d[0] * N[r, 0][:, None] + d[1] * N[r, 1][:, None] + d[2] * N[r, 2][:, None] < 0.0)
            turn = 1.0 - N[r] @ N[c].T
            close = 1.0 - np.sqrt(np.where(behind, r2, 0.0)) / R
            out["crest"][r] = np.where(behind, turn * close, 0.0).sum(axis=1)
    return out


def undecided(ref, offset, rel=1e-4):
    """Rows whose reference offsetRatio lies within a relative `rel` of the threshold: fp32 may flag them the other way."""
    return np.abs(ref["ratio"] - offset) <= rel * offset
