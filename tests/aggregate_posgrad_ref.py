"""What the tests of the position gradients of the neighbourhood sums share (include/sph_abi.h "position gradients of the neighbourhood
sums"): the pair terms restated in float64 over the relation of pkg.neighbors_host (through aggregate_ref.edges:
the fp32 acceptance, so a pair at r ~ R cannot differ in membership), their sums into the gradients, the bound of the comparison with
the fp32 twin, and a dense torch float64 forward whose autograd pins the signs independently of the pair terms.

The definition.  For target i and accepted candidate j != i, in float64 from the fp32 positions: d = x_j - x_i, r2 = d . d,
t = R2 - r2 with R2 = fl32(R * R) (the number the engine compares with), w = 1 or t^3, w1 = 0 or -6 t^2; val_c = v[j][c] (- v[i][c] with
DELTA); s_p = sum_c g[i][p][c] val_c; q = s_0 (+ d . s_{1..3} with MOMENTS); e_a = w1 q d_a (+ w s_{1+a}).  Query targets:
gradPoints[i] = -sum_j e(i -> j), gradParticles[k] = sum_i e(i -> k).  Particle targets: grad[k] = sum_j (e(j -> k) - e(k -> j)).

The bound, first order in u = 2^-24.  Write S_p = sum_c |g[i][p][c]| |val_c| and Q = S_0 (+ |d| . S_{1..3}).  On the path of one term the
twin rounds: val (1, DELTA), the channel dot (one product, ceil(C / G) lane adds and log2 G butterfly adds: `depth` roundings, each
relative to partial sums of magnitude at most S_p: gamma_depth S_p by Higham section 4.2), d_a (1), the products and sums of q (5 in
all with d's), f = w1 * q (1), f * d_a (1), w * s (1), their sum (1), and the two directions' difference (1, particle targets): at
most depth + 12 roundings relative to M_a = |w1| Q |d_a| + |w| S_{1+a}, the sum of the magnitudes of everything a term is made of.  The
weight needs an absolute term: fl32(r2) carries at most 5 u r2 (two roundings in every square, three sums) and t = R2 - r2 cancels, so
|dt| <= u t + 5 u r2, |d(t^2)| <= 2 t |dt| + 2 u t^2 <= 10 u t R2 (t + r2 = R2) and |d(t^3)| <= 3 t^2 |dt| + 2 u t^3 <= 15 u t^2 R2;
with the factors 6 and 1: X_a = 60 u t R2 Q |d_a| + 15 u t^2 R2 S_{1+a}.  A row's accumulator adds k terms: gamma_k times the sum of
their magnitudes more.  Per output component
    |twin - float64| <= gamma_(depth + 12 + k) * sum M_a + sum X_a
with k the number of terms of that row.  The same bound covers the net gradient (the sum over all rows, which is zero in exact
arithmetic because every pair term enters twice with opposite signs): it is at most the sum of the rows' bounds.

MEAN (autograd.py) is two such calls: posgrad(values, g / W) and, for the poly6 weight, a one-channel posgrad of ones with the
upstream -sum_c (g / W)[i][c] out[i][c].  mean_bound adds the two calls' bounds, each for its upstream in float64 (W from the fp32
forward, out from the float64 dense forward).  The rounding of the fp32 upstreams themselves is not added; the figures the tests
print say how much of the bound is used."""
import numpy as np

import aggregate_ref as AR

F = np.float32
U24 = 2.0 ** -24


def group(C):
    return 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32 if C <= 32 else 64


def depth(C, delta):
    G = group(C)
    return 1 + (C + G - 1) // G + int(np.log2(G)) + (1 if delta else 0)


def pair_terms(pkg, rec, sp, values, g, radius, points=None, weight="one", fluid_only=False, delta=False, moments=False, chunk=20000):
    """(rows, recv, send, e float64 (E, 3), M float64 (E, 3), X float64 (E, 3)) over the accepted pairs without the own slots."""
    rows, recv, send, _, _ = AR.edges(pkg, rec, sp, radius, points, False, fluid_only)
    n = len(rec)
    planes = 4 if moments else 1
    x = np.asarray(values, np.float64).reshape(n, -1)
    gg = np.asarray(g, np.float64).reshape(rows, planes, -1)
    pos = rec["pos"][:, :3].astype(np.float64)
    tgt = pos if points is None else np.asarray(points, F)[:, :3].astype(np.float64)
    R2 = float(F(radius) * F(radius))
    E = len(recv)
    e, M, X = np.zeros((E, 3)), np.zeros((E, 3)), np.zeros((E, 3))
    for lo in range(0, E, chunk):
        r, s_ = recv[lo:lo + chunk], send[lo:lo + chunk]
        val = x[s_] - x[r] if delta else x[s_]
        s = np.einsum("epc,ec->ep", gg[r], val)
        S = np.einsum("epc,ec->ep", np.abs(gg[r]), np.abs(val))
        d = pos[s_] - tgt[r]
        r2 = (d * d).sum(axis=1)
        t = R2 - r2
        w, w1 = (np.ones_like(t), np.zeros_like(t)) if weight == "one" else (t ** 3, -6.0 * t ** 2)
        q, Q = s[:, 0].copy(), S[:, 0].copy()
        if moments:
            q += (d * s[:, 1:]).sum(axis=1)
            Q += (np.abs(d) * S[:, 1:]).sum(axis=1)
        ee = (w1 * q)[:, None] * d
        mm = (np.abs(w1) * Q)[:, None] * np.abs(d)
        xx = np.zeros_like(ee)
        if weight != "one":
            xx = (60.0 * U24 * np.abs(t) * R2 * Q)[:, None] * np.abs(d)
        if moments:
            ee += w[:, None] * s[:, 1:]
            mm += np.abs(w)[:, None] * S[:, 1:]
            if weight != "one":
                xx += (15.0 * U24 * t * t * R2)[:, None] * S[:, 1:]
        e[lo:lo + chunk], M[lo:lo + chunk], X[lo:lo + chunk] = ee, mm, xx
    return rows, recv, send, e, M, X


def position_grad(pkg, rec, sp, values, g, radius, points=None, weight="one", fluid_only=False, delta=False, moments=False):
    """The float64 gradients and their bounds: particle targets (grad (n, 3), bound (n, 3)); query targets ((gradPoints, gradParticles),
    (boundPoints, boundParticles))."""
    n = len(rec)
    C = np.asarray(values).reshape(n, -1).shape[1]
    rows, recv, send, e, M, X = pair_terms(pkg, rec, sp, values, g, radius, points, weight, fluid_only, delta, moments)
    dep = depth(C, delta) + 12

    def gather(index, size, sign):
        out, mag, ext = np.zeros((size, 3)), np.zeros((size, 3)), np.zeros((size, 3))
        np.add.at(out, index, sign * e)
        np.add.at(mag, index, M)
        np.add.at(ext, index, X)
        return out, mag, ext, np.bincount(index, minlength=size).astype(np.float64)

    if points is None:
        a, ma, xa, ka = gather(send, n, 1.0)
        b, mb, xb, kb = gather(recv, n, -1.0)
        return a + b, AR.gamma(dep + ka + kb)[:, None] * (ma + mb) + xa + xb
    p, mp, xp, kp = gather(recv, rows, -1.0)
    q, mq, xq, kq = gather(send, n, 1.0)
    return (p, q), (AR.gamma(dep + kp)[:, None] * mp + xp, AR.gamma(dep + kq)[:, None] * mq + xq)


def mean_bound(pkg, rec, sp, values, g, out64, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False):
    """The bound of MEAN's position gradient (module docstring): particle targets (n, 3); query targets (boundPoints, boundParticles).
    out64: the float64 mean, (rows, C)."""
    n = len(rec)
    W = pkg.aggregate_host(rec, sp, np.ones((n, 1), F), radius, points=points, weight=weight, self_=self_, fluid_only=fluid_only).astype(np.float64).reshape(-1)
    gW = np.where(W[:, None] != 0, np.asarray(g, np.float64) / np.where(W != 0, W, 1.0)[:, None], 0.0)
    b = position_grad(pkg, rec, sp, values, gW, radius, points=points, weight=weight, fluid_only=fluid_only, delta=delta)[1]
    if weight == "one":
        return b
    up = -(gW * np.asarray(out64, np.float64).reshape(gW.shape)).sum(axis=1, keepdims=True)
    b2 = position_grad(pkg, rec, sp, np.ones((n, 1), F), up, radius, points=points, weight=weight, fluid_only=fluid_only)[1]
    return b + b2 if points is None else (b[0] + b2[0], b[1] + b2[1])


def dense_autograd(pkg, rec, sp, values, g, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False, op="sum"):
    """torch float64 autograd of a dense forward with the positions (and the points) as leaves and the acceptance mask detached:
    (grad of the particles' positions (n, 3), grad of the points (m, 3) or None, out), numpy float64.  op "sum" or "mean"."""
    import torch
    n = len(rec)
    rows, recv, send, _, _ = AR.edges(pkg, rec, sp, radius, points, self_, fluid_only)     # (an own slot has d = 0 and no gradient)
    mask = torch.zeros((rows, n), dtype=torch.float64)
    mask[torch.from_numpy(recv), torch.from_numpy(send)] = 1.0
    P = torch.tensor(rec["pos"][:, :3].astype(np.float64), requires_grad=True)
    T = P if points is None else torch.tensor(np.asarray(points, F)[:, :3].astype(np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(values, np.float64).reshape(n, -1))
    gt = torch.tensor(np.asarray(g, np.float64).reshape(rows, 4 if moments else 1, -1))
    d = P[None, :, :] - T[:, None, :]                                                   # (rows, n, 3): x_j - x_i
    r2 = (d * d).sum(dim=2)
    R2 = float(F(radius) * F(radius))
    w = mask + 0.0 * r2 if weight == "one" else mask * (R2 - r2) ** 3            # (0 * r2: a graph also where nothing depends on it)
    val = x[None, :, :] - x[:, None, :] if delta else x[None, :, :].expand(rows, n, x.shape[1])
    planes = [torch.einsum("ij,ijc->ic", w, val)]
    if moments:
        planes += [torch.einsum("ij,ijc->ic", w * d[:, :, a], val) for a in range(3)]
    out = torch.stack(planes, dim=1)
    if op == "mean":
        W = w.sum(dim=1)
        out = torch.where((W != 0)[:, None, None], out / torch.where(W != 0, W, torch.ones_like(W))[:, None, None], torch.zeros_like(out))
    (out * gt).sum().backward()
    return P.grad.numpy(), None if points is None else T.grad.numpy(), out.detach().numpy()
