"""The filter-grid basis sums and their adjoint on the CPU (the host twins of include/sph_abi.h "filter-grid basis sums"; DESIGN.md
section 3w): the twins against the numpy restatement conv_ref byte for byte on the query scenes; the float64 brute force; partition of
unity; constant filters; the edge of the filter grid; the transpose; the refusals and the struct layout.  No GPU is needed.

The bounds.  u = 2^-24, gamma_m = m u / (1 - m u).  A forward accumulator of row i takes k = count[i] terms coef * v in sequence: k - 1
sums and one product each, gamma_k relative to sum |coef v| when the coefficients enter the reference as the fp32 numbers the definition
rounds them to (the accumulation bound, test_aggregate_cpu's for SUM, with its two spare units: gamma_(k + 2)).  The coefficient itself,
coef = fl(w * fl(fl(wx * wy) * wz)), carries three more roundings on the term's path: gamma_(k + 3) against exact products of the hat
weights.  The hat weights are not relatively accurate, and cannot be: hi = g - i is exact given g, but g carries the absolute error of
    d = fl(x_j - x_i)   |error| <= u |d| <= u R
    q = fl(d / R)       total <= 2 u             (|q| < 1)
    t = fl(q + 1)       total <= 4 u             (t <= 2)
    g = fl(t * half)    total <= 4 u half + u (K - 1) = 3 (K - 1) u
and lo = fl(1 - f) one more u, so a hat weight is within eps = (3 (K - 1) + 2) u of the hat function at the exact coordinate (one
spare unit for the second-order terms; the hat function has slope 1, and a coordinate that crosses a cell boundary changes the cell
but not the value).  Three weights of at most 1 each: the product is within E = (1 + eps)^3 - 1 of the exact one, on every plane within
reach of the candidate.  Hence, against a float64 restatement that takes the geometry from float64 positions and w as the fp32 number,
    |A_fp32 - A_64| <= gamma_(k + 3) * sum_j |w v| (phi_b + E) + E * sum_j |w v|     (the sums over the candidates within reach of b).
The weight w stays the fp32 number in every reference, as in test_aggregate_cpu: t = R2 - r2 cancels next to the radius, so w has no
relative accuracy against float64 positions, and the fused call adds nothing to that."""
import ctypes as C

import numpy as np
import pytest

import aggregate_ref as AR
from aggregate_ref import radius_of, values_for
import conv_ref as CR
from conv_ref import PARTICLE_CASES, QUERY_CASES, U, gamma, same
import neighbors_ref as NR
import query_scenes as QS
from support import c_layout, records

F = np.float32
vp = C.c_void_p


def check_cases(pkg, rec, sp, cases, what, points=None, fluid_only=False):
    rows = len(rec) if points is None else len(points)
    for K, weight, self_, fac, c in cases:
        R = radius_of(sp, fac)
        kw = dict(points=points, size=K, weight=weight, self_=self_, fluid_only=fluid_only)
        x, h = values_for(len(rec), c), CR.planes_for(rows, K, c)
        got, cnt = pkg.aggregate_basis_host(rec, sp, x, R, counts=True, **kw)
        want, wcnt = CR.basis(pkg, rec, sp, x, R, **kw)
        tag = f"{what} {kw['size']} {weight} self {self_} fluid_only {fluid_only} R {fac} h C {c}"
        same(got, want, "forward " + tag), same(cnt, wcnt, "counts " + tag)
        assert cnt.tobytes() == pkg.aggregate_host(rec, sp, x, R, points=points, weight=weight, self_=self_, fluid_only=fluid_only, counts=True)[1].tobytes(), tag
        same(pkg.aggregate_basis_adjoint_host(rec, sp, h, R, **kw), CR.basis_adjoint(pkg, rec, sp, h, R, **kw), "adjoint " + tag)


def test_uniform(pkg):
    check_cases(pkg, *QS.uniform(pkg, 1000, 21), PARTICLE_CASES, "uniform")


def test_lattice_with_exact_ties(pkg):
    check_cases(pkg, *QS.lattice(pkg), PARTICLE_CASES, "lattice")


def test_coincident_particles(pkg):
    rec, sp, where = QS.coincident(pkg)
    check_cases(pkg, rec, sp, PARTICLE_CASES, "coincident")
    out = pkg.aggregate_basis_host(rec, sp, np.ones(len(rec), F), 1.0, size=3, weight="one")
    assert (out[where, 13, 0] >= 7).all()                                               # the seven others at d = 0: the centre cell


@pytest.mark.parametrize("fluid_only", [False, True])
def test_ghosts(pkg, fluid_only):
    rec, sp = QS.with_ghosts(pkg)
    check_cases(pkg, rec, sp, PARTICLE_CASES, "ghosts", fluid_only=fluid_only)
    check_cases(pkg, rec, sp, QUERY_CASES[:3], "ghosts, query", points=rec["pos"][:333, :3].copy(), fluid_only=fluid_only)
    if fluid_only:
        ghost = rec["isGhost"] != 0
        out = pkg.aggregate_basis_host(rec, sp, values_for(len(rec), 2), 1.0, size=2, self_=True, fluid_only=True)
        adj = pkg.aggregate_basis_adjoint_host(rec, sp, CR.planes_for(len(rec), 2, 2), 1.0, size=2, self_=True, fluid_only=True)
        assert (out[ghost].view(np.uint32) == 0).all() and (adj[ghost].view(np.uint32) == 0).all() and out[~ghost].any() and adj[~ghost].any()


def test_crowded_cell(pkg):
    rec, sp, start, members = QS.crowded_cell(pkg, 200)
    check_cases(pkg, rec, sp, PARTICLE_CASES[1:4], "crowd 200")


def test_query_cloud_and_non_finite_records(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    assert not NR.inside_grid(pkg, rec["pos"], sp)                                      # clamped cells take part
    check_cases(pkg, rec, sp, QUERY_CASES, "query cloud", points=pts)
    gone = [5, 256, 700]                                                                # the three non-finite points
    out, cnt = pkg.aggregate_basis_host(rec, sp, values_for(len(rec), 3), 1.0, points=pts, size=3, counts=True)
    assert (cnt[gone] == 0).all() and (out[gone].view(np.uint32) == 0).all() and cnt.sum() > 0
    h = CR.planes_for(len(pts), 3, 3)
    h2 = h.copy()
    h2[gone] = 1000.0
    same(pkg.aggregate_basis_adjoint_host(rec, sp, h2, 1.0, points=pts, size=3), pkg.aggregate_basis_adjoint_host(rec, sp, h, 1.0, points=pts, size=3), "non-finite points")
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    check_cases(pkg, rec, sp, PARTICLE_CASES[:4], "non-finite positions")
    x = values_for(len(rec), 2)
    out, cnt = pkg.aggregate_basis_host(rec, sp, x, 1.0, size=4, counts=True)
    assert cnt[7] == 0 and cnt[300] == 0 and not out[[7, 300]].any()
    # NaN and inf values reach the rows that accept them, and no other row
    x2 = x.copy()
    x2[11, 0], x2[12, 1] = np.nan, np.inf
    off, idx = pkg.neighbors_host(rec, sp, 1.0)
    sees = lambda j: np.array([j in idx[off[i]:off[i + 1]] for i in range(len(rec))])
    dirty = pkg.aggregate_basis_host(rec, sp, x2, 1.0, size=4)
    assert np.isnan(dirty[sees(11), :, 0]).any(axis=1).all() and not np.isfinite(dirty[sees(12), :, 1]).all(axis=1).any()
    assert np.array_equal(dirty[~sees(11), :, 0].view(np.uint32), out[~sees(11), :, 0].view(np.uint32))
    same(dirty, CR.basis(pkg, rec, sp, x2, 1.0, size=4)[0], "NaN values")


def float64_pieces(pkg, rec, sp, R, K, weight):
    """Over the float64 brute-force pairs (no grid): (offsets of the rows, recv, send, w as the fp32 numbers, phi (E, B) the exact
    trilinear hats of the float64 offsets, reach (E, B): the planes within one cell of the candidate on every axis)."""
    off, idx, margin = NR.brute_force(pkg, rec["pos"], sp, R)
    assert margin > 1e-6, "a pair so close to the radius that fp32 and float64 may disagree about it"
    rows, recv, send, d, r2 = AR.edges(pkg, rec, sp, R)
    assert np.array_equal(send, idx) and np.array_equal(np.bincount(recv, minlength=rows), np.diff(off))      # the same pairs in the same order
    X = rec["pos"][:, :3].astype(np.float64)
    g = ((X[send] - X[recv]) / float(F(R)) + 1.0) * (0.5 * (K - 1))                     # (E, 3)
    dist = np.abs(g[:, :, None] - np.arange(K)[None, None, :])                          # (E, 3, K)
    hat, near = np.maximum(0.0, 1.0 - dist), dist <= 1.0 + 1e-6
    phi = (hat[:, 2, :, None, None] * hat[:, 1, None, :, None] * hat[:, 0, None, None, :]).reshape(len(g), -1)
    reach = (near[:, 2, :, None, None] & near[:, 1, None, :, None] & near[:, 0, None, None, :]).reshape(len(g), -1)
    return off, recv, send, AR.weights(weight, R, r2).astype(np.float64), phi, reach


def row_sums(off, terms):
    """terms (E, ...) summed over the edges of every row (float64)."""
    out = np.zeros((len(off) - 1,) + terms.shape[1:])
    full = np.diff(off) > 0
    if len(terms):
        out[full] = np.add.reduceat(terms, off[:-1][full], axis=0)
    return out


@pytest.mark.parametrize("K,weight,fac", [(2, "one", 1.0), (3, "poly6", 2.0), (4, "poly6", 1.0), (4, "one", 2.0)])
def test_within_the_float64_bounds(pkg, K, weight, fac):
    """Against the all-pairs float64 restatement: first the accumulation alone (the fp32 coefficients summed in float64, gamma_(k + 2)
    of sum |coef v|), then the whole path with the geometry in float64 (the module docstring's bound)."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    R, c = radius_of(sp, fac), 3
    x = values_for(len(rec), c)
    got, cnt = pkg.aggregate_basis_host(rec, sp, x, R, size=K, weight=weight, counts=True)
    off, recv, send, w, phi, reach = float64_pieces(pkg, rec, sp, R, K, weight)
    k = cnt.astype(np.float64)
    # the accumulation
    T = CR.dense(pkg, rec, sp, R, size=K, weight=weight)                                # (rows, B, n): the fp32 coefficients
    s64, a64 = np.einsum("ibk,kc->ibc", T, x.astype(np.float64)), np.einsum("ibk,kc->ibc", np.abs(T), np.abs(x).astype(np.float64))
    err, bound = np.abs(got - s64), gamma(k + 2)[:, None, None] * a64
    acc_ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    assert (err <= bound).all()
    # the whole path
    xs = x[send].astype(np.float64)
    s64 = row_sums(off, (w[:, None] * phi)[:, :, None] * xs[:, None, :])
    mag = row_sums(off, (w[:, None] * phi)[:, :, None] * np.abs(xs)[:, None, :])
    absmag = row_sums(off, (w[:, None] * reach)[:, :, None] * np.abs(xs)[:, None, :])
    E = (1.0 + (3 * (K - 1) + 2) * U) ** 3 - 1.0
    err, bound = np.abs(got - s64), gamma(k + 3)[:, None, None] * (mag + E * absmag) + E * absmag
    print(f"K {K} {weight} R {fac} h: largest error / bound, accumulation {acc_ratio:.3g}, whole path {np.max(err / np.maximum(bound, 1e-300)):.3g}, "
          f"mean count {cnt.mean():.1f}")
    assert (err <= bound).all() and (got[bound == 0] == 0).all()


@pytest.mark.parametrize("K,weight,self_,fac", [(2, "one", False, 1.0), (3, "poly6", True, 2.0), (4, "poly6", False, 1.0), (4, "one", True, 3.0)])
def test_partition_of_unity(pkg, K, weight, self_, fac):
    """sum_b A[i][b][c] is the plain SUM: the hats of a candidate add up to one.  In fp32 lo + hi = fl(1 - f) + f is within u of 1 per
    axis and every coefficient carries three roundings, so sum_b coef = w (1 + delta), |delta| <= 6 u (1 + ...) <= gamma_7; the planes
    are within gamma_(k + 2) of their own magnitudes (the accumulation bound) and so is the SUM."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    R, c = radius_of(sp, fac), 5
    x = values_for(len(rec), c)
    A, cnt = pkg.aggregate_basis_host(rec, sp, x, R, size=K, weight=weight, self_=self_, counts=True)
    S = pkg.aggregate_host(rec, sp, x, R, weight=weight, self_=self_)
    T = CR.dense(pkg, rec, sp, R, size=K, weight=weight, self_=self_)
    mag_planes = np.einsum("ibk,kc->ic", np.abs(T), np.abs(x).astype(np.float64))
    mag_sum = np.abs(AR.aggregate(pkg, rec, sp, np.abs(x), R, weight=weight, self_=self_)[0].astype(np.float64)) / (1.0 - gamma(cnt + 2.0))[:, None]
    k = cnt.astype(np.float64)
    err = np.abs(A.astype(np.float64).sum(axis=1) - S)
    bound = gamma(k + 2)[:, None] * mag_planes + (gamma(k + 2) + gamma(7.0))[:, None] * mag_sum
    print(f"K {K} {weight} self {self_} R {fac} h: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all() and mag_sum.any()


def test_constant_filters(pkg):
    """Filters that are the same Cin x Cout matrix M in every cell: continuous_conv is aggregate SUM @ M.  Elementwise the partition
    bound of every input channel times |M|, plus the matrix product of B * Cin terms per output, gamma_(B Cin) of sum |A| |M| in any
    order of summation, fused or not."""
    import torch
    rec, sp = QS.uniform(pkg, 600, 21)
    host = pkg.HostAggregateBackend(rec, sp)
    rng = np.random.default_rng(3)
    for K, weight, self_, fac, cin, cout in ((3, "poly6", True, 2.0, 4, 3), (4, "one", False, 1.0, 3, 5)):
        R = radius_of(sp, fac)
        x, M = values_for(len(rec), cin), rng.normal(0.0, 1.0, (cin, cout)).astype(F)
        filt = np.broadcast_to(M, (K, K, K, cin, cout)).copy()
        y = pkg.continuous_conv(host, None, torch.from_numpy(x), torch.from_numpy(filt), R, weight=weight, self_=self_).numpy()
        A, cnt = pkg.aggregate_basis_host(rec, sp, x, R, size=K, weight=weight, self_=self_, counts=True)
        S = pkg.aggregate_host(rec, sp, x, R, weight=weight, self_=self_).astype(np.float64)
        T = CR.dense(pkg, rec, sp, R, size=K, weight=weight, self_=self_)
        k = cnt.astype(np.float64)
        mag = np.einsum("ibk,kc->ic", np.abs(T), np.abs(x).astype(np.float64))         # (the SUM's magnitudes are at most these times 1 + gamma_7)
        partition = (2.0 * gamma(k + 2) + gamma(7.0))[:, None] * mag * (1.0 + gamma(7.0))
        absM = np.abs(M).astype(np.float64)
        bound = partition @ absM + gamma(K ** 3 * cin + 1.0) * (np.abs(A).astype(np.float64).sum(axis=1) @ absM)
        err = np.abs(y - S @ M.astype(np.float64))
        print(f"K {K} {weight}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, |M| max {absM.max():.3g}")
        assert y.shape == (len(rec), cout) and (err <= bound).all() and S.any()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_edge_of_the_filter_grid(pkg, K):
    """A pair one ulp inside R along x: from the left particle the offset is +d (g_x rounds to K - 1, cell K - 2 with hi = 1), from the
    right one -d (g_x = 2^-24 half, cell 0).  Every coefficient lands inside [0, B) and they add up to w."""
    sp = QS.params(pkg)
    R = F(sp.param_h)
    d = np.nextafter(R, F(0))
    pos = np.array([[0.0, -0.5, 0.0], [d, -0.5, 0.0], [1.5, 0.75, 1.0]], F)             # (the third is alone)
    rec = records(pkg, pos, np.zeros_like(pos))
    ones = np.ones((3, 1), F)
    i, lo, hi = CR.axis(np.array([d, -d], F), R, K)
    assert i.tolist() == [K - 2, 0] and hi[0] == 1 and lo[0] == 0 and 1 - 2.0 ** -23 <= lo[1] <= 1 and 0 < hi[1] <= 1.5 * 2.0 ** -24
    for weight in ("one", "poly6"):
        buf = np.full(3 * K ** 3 + 64, 7.0, F)
        out = buf[32:32 + 3 * K ** 3]
        cfg = pkg.basis_config(radius=float(R), size=K, channels=1, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6 if weight == "poly6" else pkg.SPH_AGGREGATE_WEIGHT_ONE)
        assert pkg.load_library().sph_aggregate_basis_host(rec.ctypes.data_as(vp), 3, C.byref(sp), C.byref(cfg), None, 0, ones.ctypes.data_as(vp),
                                                           out.ctypes.data_as(vp), None) == 0
        assert (buf[:32] == 7.0).all() and (buf[32 + 3 * K ** 3:] == 7.0).all()         # nothing lands outside the rows
        A = out.reshape(3, K, K, K).copy()                                              # [row][z][y][x]
        same(A.reshape(3, K ** 3, 1), CR.basis(pkg, rec, sp, ones, float(R), size=K, weight=weight)[0], f"edge {weight}")
        w = float(AR.weights(weight, float(R), np.array([d * d], F))[0])
        assert w > 0 and not A[2].any()
        assert not A[0, :, :, :K - 1].any() and abs(A[0].sum(dtype=np.float64) - w) <= gamma(4.0) * w      # all of it on the last x plane
        assert not A[1, :, :, 2:].any() and A[1, :, :, 0].sum() > 0.999 * w and abs(A[1].sum(dtype=np.float64) - w) <= gamma(8.0) * w
    if K == 3:                                                                          # the own slot: wholly the centre cell, with coefficient w
        x = np.array([[2.0, -3.0], [0.5, 0.25], [4.0, -1.0]], F)
        A = pkg.aggregate_basis_host(rec, sp, x, float(R), size=3, weight="poly6", self_=True)
        w0 = AR.weights("poly6", float(R), np.zeros(1, F))[0]
        assert np.array_equal(A[2, 13], (w0 * x[2]).astype(F)) and (np.delete(A[2], 13, axis=0).view(np.uint32) == 0).all()
        one = pkg.aggregate_basis_host(rec, sp, x, float(R), size=3, weight="one", self_=True)
        assert np.array_equal(one[2, 13], x[2]) and np.array_equal(one[0, 13], x[0])


TRANSPOSE_CASES = [(K, weight, self_, fluid_only, c) for (K, weight), (self_, fluid_only), c in
                   zip([(2, "one"), (3, "poly6"), (4, "poly6"), (3, "one"), (4, "one"), (2, "poly6")] * 2,
                       [(False, False), (True, False), (False, True), (True, True)] * 3, [1, 3, 16] * 4)]


def check_transpose(pkg, rec, sp, K, weight, self_, fluid_only, c, what, points=None):
    """<A x, h> = <x, A^T h>, both sides accumulated in float64.  With A the matrix of the fp32 coefficients the identity is exact, a
    forward accumulator carries gamma_kf (kf terms: kf - 1 sums and the product) and an adjoint accumulator gamma_(8 ka) (8 corners of
    each of ka rows), so the difference is at most (gamma_(kf + 2) + gamma_(8 ka + 2)) T, T the sum of |coef| |x| |h| over every term,
    kf and ka the largest counts; the two spare units cover the float64 inner products."""
    rows = len(rec) if points is None else len(points)
    R = radius_of(sp, 2.0)
    kw = dict(points=points, size=K, weight=weight, self_=self_, fluid_only=fluid_only)
    x = values_for(len(rec), c, seed=41)
    h = CR.planes_for(rows, K, c, seed=43)
    if points is not None:
        h[~np.isfinite(points).all(axis=1)] = 0.0
    y = pkg.aggregate_basis_host(rec, sp, x, R, **kw)
    z = pkg.aggregate_basis_adjoint_host(rec, sp, h, R, **kw)
    lhs = float((y.astype(np.float64) * h.astype(np.float64)).sum())
    rhs = float((x.astype(np.float64) * z.astype(np.float64)).sum())
    rows_, recv, send, b, coef, w = CR.terms(pkg, rec, sp, R, **kw)
    T = float((np.abs(coef.astype(np.float64))[:, :, None] * np.abs(x[send].astype(np.float64))[:, None, :] * np.abs(h[recv[:, None], b].astype(np.float64))).sum())
    kf, ka = int(np.bincount(recv, minlength=1).max()), int(np.bincount(send, minlength=1).max())
    bound = float(gamma(kf + 2.0) + gamma(8.0 * ka + 2.0)) * T
    print(f"{what} {kw['size']} {weight} self {self_} fluid_only {fluid_only} C {c}: <Ax, h> {lhs:.9g}, <x, A^T h> {rhs:.9g}, |difference| / bound "
          f"{abs(lhs - rhs) / bound:.3g}, kf {kf} ka {ka}")
    assert T > 0 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=str)
def test_transpose_particles(pkg, case):
    rec, sp = QS.with_ghosts(pkg)
    check_transpose(pkg, rec, sp, *case, "ghosts")


@pytest.mark.parametrize("case", [c for c in TRANSPOSE_CASES if not c[2]], ids=str)
def test_transpose_query(pkg, case):
    rec, sp, pts = QS.query_cloud(pkg)
    rec["isGhost"] = np.arange(len(rec)) % 3 == 0
    check_transpose(pkg, rec, sp, *case, "query cloud", points=pts)


def test_refusals_write_nothing(pkg):
    """Every SPH_ERR_ARG case of include/sph_abi.h by name, but one: rows * B * channels beyond size_t cannot be reached through a
    64-bit size_t (rows <= 2^31 - 1 or the engine's particle limit, B * channels <= 8192); the check stays in the library."""
    L = pkg.load_library()
    rec, sp = QS.uniform(pkg, 50, 3)
    n, h = len(rec), sp.param_h
    x = values_for(n, 4)
    pts = np.zeros((3, 4), F)
    out, cnt, back = np.full((n, 8, 4), 7.0, F), np.full(n, 9, np.uint32), np.full((n, 4), 7.0, F)
    hp, hq = np.zeros((n, 8, 4), F), np.zeros((3, 8, 4), F)                             # h of particle rows and of the three query points
    p = lambda a: None if a is None else a.ctypes.data_as(vp)

    def forward(cfg, points=None, m=0, values=x, out_=out, cnt_=cnt, params=sp, cfg_null=False):
        rc = L.sph_aggregate_basis_host(p(rec), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg), p(points), m, p(values),
                                        p(out_), p(cnt_))
        assert (out == 7.0).all() and (cnt == 9).all()
        return rc

    def adjoint(cfg, points=None, m=0, h_="rows", out_=back, params=sp, cfg_null=False):
        h_ = (hp if points is None else hq) if isinstance(h_, str) else h_
        rc = L.sph_aggregate_basis_adjoint_host(p(rec), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg), p(points), m,
                                                p(h_), p(out_))
        assert (back == 7.0).all()
        return rc

    good = dict(radius=h, channels=4, size=2)
    for call in (forward, adjoint):
        assert call(pkg.basis_config(**good), cfg_null=True) == -1 and call(pkg.basis_config(**good), params=None) == -1, "a null argument"
        assert call(pkg.basis_config(**good), out_=None) == -1, "a null output"
        for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
            assert call(pkg.basis_config(**dict(good, radius=R))) == -1, f"radius {R}"
        for name, bad in (("an unknown weight", dict(weight=-1)), ("an unknown weight", dict(weight=2)), ("DELTA", dict(flags=pkg.SPH_AGGREGATE_DELTA)),
                          ("MOMENTS", dict(flags=pkg.SPH_AGGREGATE_MOMENTS)), ("DELTA with SELF", dict(flags=pkg.SPH_AGGREGATE_DELTA | pkg.SPH_AGGREGATE_SELF)),
                          ("an unknown flag bit", dict(flags=16)), ("no channel", dict(channels=0)), ("129 channels", dict(channels=129)),
                          ("negative channels", dict(channels=-3)), ("an unknown kind", dict(kind=1)), ("an unknown kind", dict(kind=-1)), ("K = 1", dict(size=1)),
                          ("K = 5", dict(size=5)), ("K = 0", dict(size=0))):
            assert call(pkg.basis_config(**dict(good, **bad))) == -1, name
        for i in range(2):
            padded = pkg.basis_config(**good)
            padded.pad[i] = 1
            assert call(padded) == -1, "non-zero padding"
        assert call(pkg.basis_config(flags=pkg.SPH_AGGREGATE_SELF, **good), points=pts, m=3) == -1, "SELF on query targets"
        assert call(pkg.basis_config(**good), points=pts, m=1 << 31) == -1, "2^31 query points"
    assert forward(pkg.basis_config(**good), values=None) == -1 and adjoint(pkg.basis_config(**good), h_=None) == -1
    assert forward(pkg.basis_config(flags=pkg.SPH_AGGREGATE_DELTA, **good)) == -1 and b"DELTA" in L.sph_last_error()
    # overlapping address ranges: out or count with the values; the adjoint's out with h or with the points
    both = np.full(n * 32 + 8, 7.0, F)
    assert L.sph_aggregate_basis_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), None, 0, p(both[n * 32 - 8:]), p(both[:n * 32]), None) == -1
    assert (both == 7.0).all() and b"overlap" in L.sph_last_error()
    assert L.sph_aggregate_basis_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), None, 0, p(both[:n * 4]), p(out), p(both[4:].view(np.uint32))) == -1
    assert (both == 7.0).all() and (out == 7.0).all()
    assert L.sph_aggregate_basis_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), None, 0, p(both[:n * 32]), p(both[n * 32 - 8:])) == -1
    assert (both == 7.0).all() and b"overlap" in L.sph_last_error()
    big = np.full(n * 4 + 16, 7.0, F)
    assert L.sph_aggregate_basis_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), p(big[n * 4 - 4:]), 3, p(hq), p(big[:n * 4])) == -1
    assert (big == 7.0).all()
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_host(rec, sp, x, h, weight="gauss")
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_host(rec, sp, x, h, size=5)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_host(rec, sp, x[:-1], h)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_adjoint_host(rec, sp, np.zeros((n, 27, 4), F), h, size=4)   # (n, 27, C) where (n, 64, C) is due
    # the valid calls write every row and nothing else; m = 0 and n = 0 succeed
    assert L.sph_aggregate_basis_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), None, 0, p(x), p(out), p(cnt)) == 0
    same(out.copy(), pkg.aggregate_basis_host(rec, sp, x, h, size=2), "the valid call")
    assert L.sph_aggregate_basis_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.basis_config(**good)), p(pts), 0, p(hq), p(back)) == 0
    assert (back.view(np.uint32) == 0).all()                                            # m = 0: out is zeroed
    back[:] = 7.0
    assert L.sph_aggregate_basis_adjoint_host(None, 0, C.byref(sp), C.byref(pkg.basis_config(**good)), p(pts), 3, p(hq), p(back)) == 0 and (back == 7.0).all()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    assert pkg.aggregate_basis_host(none, sp, np.zeros((0, 4), F), h, size=3).shape == (0, 27, 4)
    assert pkg.aggregate_basis_host(none, sp, np.zeros((0, 4), F), h, points=np.zeros((5, 3), F)).shape == (5, 64, 4)
    assert pkg.aggregate_basis_host(rec, sp, x, h, points=np.zeros((0, 3), F), size=2).shape == (0, 8, 4)
    assert pkg.aggregate_basis_adjoint_host(none, sp, np.zeros((5, 8, 4), F), h, points=np.zeros((5, 3), F), size=2).shape == (0, 4)


def test_default_config_layout_and_abi_version(pkg, tmp_path):
    import os
    from conftest import ROOT
    cfg = pkg.basis_config()
    assert (cfg.radius, cfg.weight, cfg.flags, cfg.channels, cfg.kind, cfg.size, list(cfg.pad)) == (0.0, pkg.SPH_AGGREGATE_WEIGHT_POLY6, 0, 1, pkg.SPH_BASIS_GRID, 4, [0, 0])
    with pytest.raises(pkg.SphError):
        pkg.basis_config(pad=1)
    size, offsets, rest = c_layout("SphBasisConfig", pkg.SphBasisConfig, ['printf("%d %d\\n", SPH_BASIS_GRID, SPH_ABI_VERSION);'], tmp_path)
    assert size == C.sizeof(pkg.SphBasisConfig) == 32
    assert offsets == [(f, getattr(pkg.SphBasisConfig, f).offset) for f, _ in pkg.SphBasisConfig._fields_]
    assert [int(v) for v in rest[0].split()] == [pkg.SPH_BASIS_GRID, 4]
    with open(os.path.join(ROOT, "include", "sph_abi.h")) as fh:
        assert "#define SPH_ABI_VERSION 4 " in fh.read()                                 # additions only
