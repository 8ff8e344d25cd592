"""Brute-force float64 restatement of the anisotropic kernels (include/sph_abi.h "anisotropic kernels"): all pairs from the fp32
positions, no grid, no cells (rows and candidates are taken in the order of x, a chunk of rows against the window of candidates within
R of the chunk's x range, as shell_ref.py does), numpy.linalg.eigh in place of the Jacobi sweeps.  rows(): per particle count, the
smoothed centre, the semi-axis lengths and vectors, T = sum_k axisK axisK' (continuous in the sums: no sign or degeneracy ambiguity),
amplitude, reach and the flags, with the rows whose flags lie within rounding of a decision.  lattice(): the anisotropic fraction at
lattice nodes from those rows.  It knows nothing of stencils, so it agrees with the engine only where every particle lies inside the
grid and the largest reach stays within the stencil."""
import numpy as np

from shell_ref import EDGE, _windows

F = np.float32
VALID, SPARSE, CLAMPED = 1, 2, 4
POLY = 315.0 / (64.0 * np.pi)


def rows(pos, density, radius, support, smoothing=0.9, max_ratio=4.0, max_stretch=1.5, sparse_scale=0.5, min_count=25, exclude=None, chunk=256, rel=1e-4):
    """A dict of per-particle arrays: count, edge (a candidate within rounding of the sphere), valid, m, C (n, 3, 3), s (n, 3) after the
    clamps, raw (n, 3) before them, V (n, 3, 3) eigenvector columns, center, axes (n, 3, 3) rows = axis0 / 1 / 2, T, reach, amplitude,
    flags, undecided (a clamp decision or minCount within rounding)."""
    X = np.asarray(pos, F)[:, :3].astype(np.float64)
    n = len(X)
    R = float(F(radius))
    a = float(F(support))
    R2 = R * R
    ex = np.zeros(n, bool) if exclude is None else np.asarray(exclude, bool)
    walks = np.isfinite(X).all(axis=1) & ~ex
    cand = np.flatnonzero(walks)
    count, edge, W = np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n)
    S, M = np.zeros((n, 3)), np.zeros((n, 3, 3))
    if len(cand):
        for r, c in _windows(X[cand], X[cand], R, chunk):
            r, c = cand[r], cand[c]
            d = X[c][None, :, :] - X[r][:, None, :]
            r2 = (d * d).sum(axis=2)
            acc = r2 < R2                                                          # (the particle itself is a candidate: d = 0)
            t = np.where(acc, R2 - r2, 0.0)
            w = t * t * t
            count[r] = acc.sum(axis=1)
            edge[r] = (np.abs(R2 - r2) <= EDGE * R2).any(axis=1)
            W[r] = w.sum(axis=1)
            S[r] = (w[:, :, None] * d).sum(axis=1)
            M[r] = np.einsum("rc,rca,rcb->rab", w, d, d)
    Ws = np.where(W > 0, W, 1.0)
    m = S / Ws[:, None]
    C = (M / Ws[:, None, None] - m[:, :, None] * m[:, None, :]) * (11.0 / R2)
    lam, V = np.linalg.eigh(C)
    lam, V = lam[:, ::-1], V[:, :, ::-1]                                           # descending, columns with them
    raw = np.sqrt(np.maximum(lam, 0.0))
    sparse = walks & ((count < min_count) | ~(raw[:, 0] > 0))
    s0 = np.minimum(raw[:, 0], max_stretch)
    lo = s0 / max_ratio
    s = np.stack([s0, np.minimum(np.maximum(raw[:, 1], lo), max_stretch), np.minimum(np.maximum(raw[:, 2], lo), max_stretch)], axis=1)
    clamped = walks & ~sparse & (s != raw).any(axis=1)
    near = lambda x, y: np.abs(x - y) <= rel * np.abs(y)
    undecided = walks & ~sparse & (near(raw[:, 0], max_stretch) | near(raw[:, 1], lo) | near(raw[:, 2], lo) | near(raw[:, 1], max_stretch) |
                                   near(raw[:, 2], max_stretch))
    undecided |= walks & edge & (np.abs(count - min_count) <= 1)
    s[sparse] = sparse_scale
    V[sparse] = np.eye(3)
    s[~walks] = 0.0
    semi = a * s
    axes = semi[:, :, None] * np.swapaxes(V, 1, 2)                                  # axes[i, k] = (a s_k) v_k
    axes[~walks] = 0.0
    center = np.where(walks[:, None], X + smoothing * m, 0.0)
    rho = np.asarray(density, F).astype(np.float64)
    inv = np.where(rho > 0, 1.0 / np.where(rho > 0, rho, 1.0), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        amplitude = np.where(walks, inv / np.where(walks, semi.prod(axis=1), 1.0), 0.0)
        Q = np.einsum("ik,iak,ibk->iab", np.where(walks[:, None], 1.0 / np.where(semi > 0, semi, 1.0) ** 2, 0.0), V, V)
    reach = np.where(walks, semi[:, 0] + np.linalg.norm(center - X, axis=1), 0.0)
    flags = np.where(walks, VALID | np.where(sparse, SPARSE, 0) | np.where(clamped, CLAMPED, 0), 0)
    return dict(count=np.where(walks, count, 0), edge=edge, valid=walks, m=m, C=C, s=s, raw=raw, V=V, center=center, axes=axes,
                T=np.einsum("ika,ikb->iab", axes, axes), reach=reach, amplitude=amplitude, Q=Q, rho2=semi[:, 0] ** 2, flags=flags,
                undecided=undecided)


def lattice(ref, mass, origin, spacing, dims, chunk=2048):
    """The anisotropic fraction (nz, ny, nx) at origin + i * spacing (fp32 coordinates as the engine forms them) from the rows of rows()."""
    nx, ny, nz = dims
    o, sp = np.asarray(origin, F), np.broadcast_to(np.asarray(spacing, F), (3,))
    ax = [(o[k] + np.arange(d, dtype=F) * sp[k]).astype(F).astype(np.float64) for k, d in enumerate((nx, ny, nz))]
    P = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]     # x fastest
    use = np.flatnonzero(ref["valid"])
    c, Q, amp, rho2 = ref["center"][use], ref["Q"][use], ref["amplitude"][use], ref["rho2"][use]
    out = np.zeros(len(P))
    for a in range(0, len(P), chunk):
        r = P[a:a + chunk, None, :] - c[None, :, :]
        near = (r * r).sum(axis=2) < rho2[None, :]
        q2 = np.einsum("pja,jab,pjb->pj", r, Q, r)
        u = np.where(near, np.maximum(1.0 - q2, 0.0), 0.0)
        out[a:a + chunk] = (u ** 3 * amp[None, :]).sum(axis=1)
    fin = np.isfinite(P).all(axis=1)
    return np.where(fin, float(F(mass)) * POLY * out, 0.0).reshape(nz, ny, nx)


def twin_T(rows_):
    """T = sum_k axisK axisK' of the twin's (or the device's) rows, in float64."""
    A = np.stack([rows_["axis0"], rows_["axis1"], rows_["axis2"]], axis=1).astype(np.float64)
    return np.einsum("ika,ikb->iab", A, A)


def level_heights(values, zs, level):
    """Per (y, x) column of a (nz, ny, nx) lattice the height where the value falls through `level`, searched from the top and linearly
    interpolated between the two nodes; NaN where the column never reaches it."""
    v = np.asarray(values, np.float64)
    nz = v.shape[0]
    out = np.full(v.shape[1:], np.nan)
    for j in range(v.shape[1]):
        for i in range(v.shape[2]):
            col = v[:, j, i]
            for l in range(nz - 2, -1, -1):
                if col[l] >= level > col[l + 1]:
                    out[j, i] = zs[l] + (zs[l + 1] - zs[l]) * (col[l] - level) / (col[l] - col[l + 1])
                    break
    return out
