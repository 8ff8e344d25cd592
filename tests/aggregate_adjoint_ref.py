"""What the tests of the adjoint of the neighbourhood sums share (include/sph_abi.h "the adjoint of the neighbourhood sums"; DESIGN.md
section 3v): the dense matrix of a SUM built from pkg.neighbors_host lists (through aggregate_ref.edges), in float64 for the bound and in
integers for the exact transpose; the two magnitude sums T of the dot-product test; the winners of MAX / MIN by their definition.

The matrix.  One channel of a SUM is out[i][p] = sum_k A[p][i][k] x[k] with, over the accepted pairs (row i, candidate k) of the lists,
A[0][i][k] = w and A[1 + a][i][k] = fl(w * d_a) (the fp32 numbers the definition rounds them to); DELTA subtracts every row's sum from
its diagonal, because the reduced value is x[k] - x[i].  The transpose is (A^T g)[k] = sum_p sum_i A[p][i][k] g[i][p].

The bound of the dot-product test.  Let y = fl(A x) and z = fl(A^T g) be the fp32 results.  Then
    <y, g> - <x, z> = <y - A x, g> + <x, A^T g - z>,
because <A x, g> = <x, A^T g> exactly.  Each component of y - A x is the error of a recursive fp32 sum of k terms, every term carrying at
most three more roundings (DELTA's subtraction, w * d_a, the product): by the standard bound (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2) it is at most gamma_(k + 3) times the sum of the terms' magnitudes, gamma_j = j u / (1 - j u),
u = 2^-24.  Summed against |g| this is gamma_(kmax + 3) * T_f, where T_f is the double sum <A x, g> with every factor replaced by its
absolute value; the same on the other side gives gamma_(kmax + 3) * T_a with the factors of <x, A^T g>.  Without DELTA the two sums
have the same factors and T_f = T_a; with DELTA the difference x[k] - x[i] is one factor of the first and g[i] -+ g[k] one factor of
the second, and T is the larger of the two.  Together
    |<y, g> - <x, z>| <= 2 gamma_(kmax + 3) T <= (kmax + 8) * 2^-23 * T
(2 u = 2^-23; the five extra units cover 1 / (1 - j u) for every row that fits in memory and the float64 arithmetic of the two inner
products, whose relative error is 2^-53 per operation).  kmax is the largest row count on either side: the most candidates of a row of
A and the most rows that accept one particle.  With MOMENTS the transpose adds the four planes of a row into ONE accumulator, so its
worst case is four times as long as the figure the bound uses; the bound is kept as stated and the measured ratio is printed."""
import numpy as np

import aggregate_ref as AR

F = np.float32
U = np.uint32


def coefficients(pkg, rec, sp, radius, points=None, weight="one", self_=False, fluid_only=False, moments=False):
    """The accepted pairs and their fp32 coefficients: (rows, recv, send, coef float32 (planes, E))."""
    rows, recv, send, d, r2 = AR.edges(pkg, rec, sp, radius, points, self_, fluid_only)
    w = AR.weights(weight, radius, r2)
    coef = [w] + ([(w * d[:, a]).astype(F) for a in range(3)] if moments else [])
    return rows, recv, send, np.stack(coef)


def dense(pkg, rec, sp, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False):
    """A as float64 of shape (planes, rows, n)."""
    rows, recv, send, coef = coefficients(pkg, rec, sp, radius, points, weight, self_, fluid_only, moments)
    A = np.zeros((len(coef), rows, len(rec)))
    for p in range(len(coef)):
        np.add.at(A[p], (recv, send), coef[p].astype(np.float64))
        if delta:
            A[p][np.arange(rows), np.arange(rows)] -= A[p].sum(axis=1)
    return A


def transpose_apply(A, g):
    """A^T g for g of (rows, C) or (rows, planes, C), in the dtype of A (int64: exact; float64: the reference of the bound)."""
    g = np.asarray(g).reshape(A.shape[1], A.shape[0], -1)
    return np.einsum("pik,ipc->kc", A, g.astype(A.dtype))


def magnitudes(pkg, rec, sp, x, g, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False):
    """(T, kmax) of the dot-product test (module docstring), in float64 from the lists."""
    rows, recv, send, coef = coefficients(pkg, rec, sp, radius, points, weight, self_, fluid_only, moments)
    x = np.asarray(x, np.float64).reshape(len(rec), -1)
    g = np.asarray(g, np.float64).reshape(rows, len(coef), -1)
    a = np.abs(coef.astype(np.float64))
    Tf = Ta = 0.0
    for p in range(len(coef)):
        xv = np.abs(x[send] - x[recv]) if delta else np.abs(x[send])
        gv = np.abs(g[recv, p] - g[send, p] if p == 0 else g[recv, p] + g[send, p]) if delta else np.abs(g[recv, p])
        Tf += float((a[p][:, None] * xv * np.abs(g[recv, p])).sum())
        Ta += float((a[p][:, None] * np.abs(x[send]) * gv).sum())
    kmax = max(int(np.bincount(recv, minlength=1).max()), int(np.bincount(send, minlength=1).max())) if len(recv) else 0
    return max(Tf, Ta), kmax


def adjoint_magnitudes(pkg, rec, sp, g, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False):
    """Per element of A^T g the sum of the magnitudes of the terms the adjoint adds, |coef| * |g[i] -+ g[k]|, float64 (n, C), and the
    number of accepting rows of every particle."""
    rows, recv, send, coef = coefficients(pkg, rec, sp, radius, points, weight, self_, fluid_only, moments)
    g = np.asarray(g, np.float64).reshape(rows, len(coef), -1)
    mag = np.zeros((len(rec), g.shape[2]))
    for p in range(len(coef)):
        gv = np.abs(g[recv, p] - g[send, p] if p == 0 else g[recv, p] + g[send, p]) if delta else np.abs(g[recv, p])
        np.add.at(mag, send, np.abs(coef[p].astype(np.float64))[:, None] * gv)
    return mag, np.bincount(send, minlength=len(rec))


def dot_bound(T, kmax):
    return (kmax + 8) * 2.0 ** -23 * T


def winners(pkg, rec, sp, values, radius, points=None, op="max", self_=False, fluid_only=False, delta=False):
    """arg int32 (rows, C) by the definition: the smallest particle id among the accepted candidates whose reduced value is not NaN and
    whose ordered key is the row's best key; -1 where there is none."""
    x = np.ascontiguousarray(values, F).reshape(len(rec), -1)
    rows, recv, send, d, r2 = AR.edges(pkg, rec, sp, radius, points, self_, fluid_only)
    with np.errstate(invalid="ignore", over="ignore"):
        val = x[send] if not delta else (x[send] - x[recv]).astype(F)
    key, nan = AR.ordered(val).reshape(val.shape), np.isnan(val)
    none = np.iinfo(np.int64).max
    arg = np.full((rows, x.shape[1]), none, np.int64)
    for c in range(x.shape[1]):
        ok = ~nan[:, c]
        if op == "max":
            best = np.full(rows, AR.LOWEST, U)
            np.maximum.at(best, recv[ok], key[ok, c])
        else:
            best = np.full(rows, AR.HIGHEST, U)
            np.minimum.at(best, recv[ok], key[ok, c])
        won = ok & (key[:, c] == best[recv])
        np.minimum.at(arg[:, c], recv[won], send[won])
    arg[arg == none] = -1
    return arg.astype(np.int32)


def route(arg, g, n):
    """out[k][c] = the sum of g[i][c] over the rows with arg[i][c] == k (float64; exact on integer-valued g)."""
    out = np.zeros((n, g.shape[1]))
    i, c = np.nonzero(arg >= 0)
    np.add.at(out, (arg[i, c], c), np.asarray(g, np.float64)[i, c])
    return out


def small_integers(shape, seed, lo=-4, hi=5):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(F)
