"""What the tests of the position gradients of the basis sums share (include/sph_abi.h "position gradients of the basis sums"; DESIGN.md
section 3y): the pair terms restated in float64 over the relation of pkg.neighbors_host (through aggregate_ref.edges: the fp32 acceptance,
so a pair at r ~ R cannot differ in membership), their sums into the gradients, the bound of the comparison with the fp32 twin, and a
dense torch float64 forward whose autograd pins the definition independently of the pair terms.

The definition.  For target i and accepted candidate j != i, in float64 from the fp32 positions: d = x_j - x_i, r2 = d . d,
t = R2 - r2 with R2 = fl32(R * R), w = 1 or t^3, w1 = 0 or -6 t^2.  Per axis g_a = (d_a / R + 1) half, the cell i_a FROM THE FP32 RULE
(conv_ref.axis on the fp32 offset, for the other direction of a particle pair on its exact negation), f = g_a - i_a, the hat weights
1 - f and f, their slopes -s and +s with s = half / R: the linear piece the engine selects, evaluated at the float64 coordinate, so no
pair has to be left out near a kink.  Corner n: hat_n = w_x w_y w_z, dx_n = s_x w_y w_z, .. ;  q = sum_c sum_n hat_n g[i][b_n][c] x[j][c],
p_a likewise with da_n;  e_a = w1 q d_a + w p_a.  Query targets: gradPoints[i] = -sum_j e(i -> j), gradParticles[k] = sum_i e(i -> k).
Particle targets: grad[k] = sum_j (e(j -> k) - e(k -> j)), e(j -> k) with g[j], x[k] and -d.

The bound, first order in u = 2^-24, from the E of section 3w (test_conv_cpu) and the gamma terms of section 3x (aggregate_posgrad_ref).
A hat weight of the twin is within eps = (3 (K - 1) + 2) u, ABSOLUTE, of the linear piece at the float64 coordinate (test_conv_cpu's
chain d, d / R, + 1, * half, 1 - f); that piece, taken in the fp32 cell, lies in [-eps, 1 + eps].  So the product of three weights is
within E3 = (1 + 2 eps)^3 - 1 of the float64 one and the product of two within E2 = (1 + 2 eps)^2 - 1, before the roundings of the
products themselves.  Write S = sum_c sum_n |g[i][b_n][c]| |x[j][c]| (the 8 planes the candidate touches),
Q = sum_c sum_n (|hat_n| + E3) |g| |x| and P_a = sum_c sum_n (|da_n| + s E2) |g| |x|.  On the path of one term the twin rounds: the slope
(1), the two products of a corner coefficient (2), u = g * x (1), coefficient * u (1), the lane's running sum (8 ceil(C / G) adds) and
the butterfly (log2 G adds): `depth` roundings relative to partial sums of magnitude at most Q or P_a; then as section 3x d_a (1),
f = w1 * q (1), f * d_a (1), w * p_a (1), their sum (1), the two directions' difference (1) and the weight's own products (at most 4):
depth + 10 in all, relative to M_a = |w1| Q |d_a| + |w| P_a.  The absolute terms: the coefficients, Y_a = |w1| |d_a| E3 S + |w| s E2 S, and
the weight, whose t = R2 - r2 cancels (section 3x): X_a = 60 u t R2 Q |d_a| + 15 u t^2 R2 P_a (poly6 only).  A row's accumulator adds
k terms: gamma_k times the sum of their magnitudes more.  Per output component
    |twin - float64| <= gamma_(depth + 10 + k) * sum M_a + sum (X_a + Y_a)
with k the number of terms of that row.  The column sums of the particle output vanish in exact arithmetic (every pair term enters
twice with opposite signs), so they are within the sum of the rows' bounds."""
import numpy as np

import aggregate_ref as AR
import conv_ref as CR
from aggregate_posgrad_ref import group

F = np.float32
U24 = 2.0 ** -24


def depth(C):
    G = group(C)
    return 5 + 8 * ((C + G - 1) // G) + int(np.log2(G))


def eps(K):
    return (3 * (K - 1) + 2) * U24


def _corner_terms(d64, d32, radius, K):
    """Per edge: planes b (E, 8) and the float64 coefficients c (E, 8, 4) = (hat, dx, dy, dz) of the piece the fp32 rule selects."""
    R, half = float(F(radius)), 0.5 * (K - 1)
    s = half / R
    idx, lo, hi = [], [], []
    for a in range(3):
        i, _, _ = CR.axis(d32[:, a], radius, K)
        f = (d64[:, a] / R + 1.0) * half - i
        idx.append(i), lo.append(1.0 - f), hi.append(f)
    E = len(d64)
    b, c = np.zeros((E, 8), np.int64), np.zeros((E, 8, 4))
    for n in range(8):
        bit = (n & 1, (n >> 1) & 1, n >> 2)
        wt = [hi[a] if bit[a] else lo[a] for a in range(3)]
        sl = [s if bit[a] else -s for a in range(3)]
        b[:, n] = ((idx[2] + bit[2]) * K + (idx[1] + bit[1])) * K + (idx[0] + bit[0])
        c[:, n, 0] = wt[0] * wt[1] * wt[2]
        c[:, n, 1] = sl[0] * wt[1] * wt[2]
        c[:, n, 2] = wt[0] * sl[1] * wt[2]
        c[:, n, 3] = wt[0] * wt[1] * sl[2]
    return b, c, s


def _direction(gg, x, rows_of_g, rows_of_x, d64, d32, radius, K, weight):
    """e, M, XY (E, 3) of e(target -> candidate): g rows rows_of_g, candidate values rows rows_of_x, offset d."""
    E3, E2 = (1.0 + 2.0 * eps(K)) ** 3 - 1.0, (1.0 + 2.0 * eps(K)) ** 2 - 1.0
    b, c, s = _corner_terms(d64, d32, radius, K)
    assert len(b) == 0 or (b.min() >= 0 and b.max() < K ** 3)
    gx = gg[rows_of_g[:, None], b] * x[rows_of_x][:, None, :]                            # (E, 8, C): g[i][b_n][c] * x[j][c]
    ax = np.abs(gx).sum(axis=2)                                                         # (E, 8)
    sums = np.einsum("enc,enk->ek", gx, c)                                              # (E, 4): q, p_x, p_y, p_z
    S = ax.sum(axis=1)
    Q = (ax * (np.abs(c[:, :, 0]) + E3)).sum(axis=1)
    P = np.stack([(ax * (np.abs(c[:, :, 1 + a]) + s * E2)).sum(axis=1) for a in range(3)], axis=1)
    R2 = float(F(radius) * F(radius))
    t = R2 - (d64 * d64).sum(axis=1)
    w, w1 = (np.ones_like(t), np.zeros_like(t)) if weight == "one" else (t ** 3, -6.0 * t ** 2)
    ad = np.abs(d64)
    e = (w1 * sums[:, 0])[:, None] * d64 + w[:, None] * sums[:, 1:]
    M = (np.abs(w1) * Q)[:, None] * ad + np.abs(w)[:, None] * P
    XY = (np.abs(w1) * E3 * S)[:, None] * ad + (np.abs(w) * s * E2 * S)[:, None]
    if weight != "one":
        XY = XY + (60.0 * U24 * np.abs(t) * R2 * Q)[:, None] * ad + (15.0 * U24 * t * t * R2)[:, None] * P
    return e, M, XY


def position_grad(pkg, rec, sp, x, g, radius, points=None, size=4, weight="poly6", fluid_only=False, chunk=4000, magnitudes=False):
    """The float64 gradients and their bounds: particle targets (grad (n, 3), bound (n, 3)); query targets ((gradPoints, gradParticles),
    (boundPoints, boundParticles)).  magnitudes: a third entry, the sums of M_a in the same shapes (what a perturbation of g by at most
    |dg| moves the gradient by, when called with g = |dg|)."""
    n, K = len(rec), size
    rows, recv, send, d32, _ = AR.edges(pkg, rec, sp, radius, points, False, fluid_only)
    x = np.asarray(x, np.float64).reshape(n, -1)
    C = x.shape[1]
    gg = np.asarray(g, np.float64).reshape(rows, K ** 3, C)
    pos = rec["pos"][:, :3].astype(np.float64)
    tgt = pos if points is None else np.asarray(points, F)[:, :3].astype(np.float64)
    dep = depth(C) + 10
    acc = {name: (np.zeros((size_, 3)), np.zeros((size_, 3)), np.zeros((size_, 3))) for name, size_ in (("points", rows), ("particles", n))}

    def add(name, index, sign, e, M, XY):
        out, mag, ext = acc[name]
        np.add.at(out, index, sign * e), np.add.at(mag, index, M), np.add.at(ext, index, XY)

    for lo in range(0, len(recv), chunk):
        r, s_ = recv[lo:lo + chunk], send[lo:lo + chunk]
        d64, dd = pos[s_] - tgt[r], np.ascontiguousarray(d32[lo:lo + chunk], F)
        out_terms = _direction(gg, x, r, s_, d64, dd, radius, K, weight)                # e(i -> j)
        if points is None:
            add("particles", r, -1.0, *out_terms)
            add("particles", r, 1.0, *_direction(gg, x, s_, r, -d64, (-dd).astype(F), radius, K, weight))     # e(j -> i), summed at i
        else:
            add("points", r, -1.0, *out_terms)
            add("particles", s_, 1.0, *out_terms)
    kp, kq = np.bincount(recv, minlength=rows).astype(np.float64), np.bincount(send, minlength=n).astype(np.float64)
    bound = lambda name, k: AR.gamma(dep + k)[:, None] * acc[name][1] + acc[name][2]
    if points is None:
        return (acc["particles"][0], bound("particles", 2.0 * kp)) + ((acc["particles"][1],) if magnitudes else ())
    return ((acc["points"][0], acc["particles"][0]), (bound("points", kp), bound("particles", kq))) + (((acc["points"][1], acc["particles"][1]),) if magnitudes else ())


def dense_autograd(pkg, rec, sp, x, g, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False, filters=None, normalize=False):
    """torch float64 autograd of a dense forward with the positions (and the points) as leaves, the acceptance mask and the cells (from
    the fp32 rule) detached: (grad of the particles' positions (n, 3), grad of the points (m, 3) or None, out), numpy float64.
    filters None: L = sum g . A, g (rows, K^3, C); else L = sum g . (A @ filters (/ W with normalize)), g (rows, Cout)."""
    import torch
    n, K = len(rec), size
    rows, recv, send, d32, _ = AR.edges(pkg, rec, sp, radius, points, self_, fluid_only)
    er, es = torch.from_numpy(recv), torch.from_numpy(send)
    P = torch.tensor(rec["pos"][:, :3].astype(np.float64), requires_grad=True)
    T = P if points is None else torch.tensor(np.asarray(points, F)[:, :3].astype(np.float64), requires_grad=True)
    xt = torch.tensor(np.asarray(x, np.float64).reshape(n, -1))
    C = xt.shape[1]
    R, half, R2 = float(F(radius)), 0.5 * (K - 1), float(F(radius) * F(radius))
    d = P[es] - T[er]                                                                   # (E, 3); an own slot (SELF) has d = x_i - x_i: no gradient
    r2 = (d * d).sum(dim=1)
    w = torch.ones_like(r2) + 0.0 * r2 if weight == "one" else (R2 - r2) ** 3
    cells = [torch.from_numpy(CR.axis(d32[:, a], radius, K)[0]) for a in range(3)]
    hi = [(d[:, a] / R + 1.0) * half - cells[a] for a in range(3)]
    A = torch.zeros((rows, K ** 3, C), dtype=torch.float64)
    for nn in range(8):
        bit = (nn & 1, (nn >> 1) & 1, nn >> 2)
        wt = [hi[a] if bit[a] else 1.0 - hi[a] for a in range(3)]
        b = ((cells[2] + bit[2]) * K + (cells[1] + bit[1])) * K + (cells[0] + bit[0])
        A = A.index_put((er, b), (w * wt[0] * wt[1] * wt[2])[:, None] * xt[es], accumulate=True)
    gt = torch.tensor(np.asarray(g, np.float64))
    if filters is None:
        out = A
    else:
        Fm = torch.tensor(np.asarray(filters, np.float64))                              # (K, K, K, Cin, Cout), axes z, y, x: plane-major rows
        out = A.reshape(rows, -1) @ Fm.reshape(K ** 3 * C, -1)
        if normalize:
            W = torch.zeros(rows, dtype=torch.float64).index_put((er,), w, accumulate=True)
            out = torch.where((W != 0)[:, None], out / torch.where(W != 0, W, torch.ones_like(W))[:, None], torch.zeros_like(out))
    (out * gt.reshape(out.shape)).sum().backward()
    return P.grad.numpy(), None if points is None else T.grad.numpy(), out.detach().numpy()


# (size K, weight, radius in h, C): every K, both weights, the three stencils, channel counts on both sides of a group and of T = 2
CASES = [
    (2, "one", 1.0, 1),
    (3, "poly6", 2.0, 3),
    (4, "poly6", 1.0, 5),
    (4, "one", 2.5, 2),
    (3, "one", 0.7, 17),
    (2, "poly6", 3.0, 3),
    (4, "poly6", 1.0, 70),
]
