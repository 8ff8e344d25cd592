"""The adjoint of the neighbourhood sums, the extrema with their winners and the routing through them on the CPU (the host twins of
include/sph_abi.h "the adjoint of the neighbourhood sums"): the exact transpose on integer data, the identities with the forward, the
dot-product test within the bound derived in aggregate_adjoint_ref, the winners by their definition, and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aggregate_adjoint_ref as AJ
import aggregate_ref as AR
from aggregate_ref import PARTICLE_CASES, QUERY_CASES, radius_of, values_for
import query_scenes as QS
from support import records

F = np.float32
vp = C.c_void_p
SUM_CASES = [c for c in PARTICLE_CASES if c[0] == "sum"]
SUM_QUERY_CASES = [c for c in QUERY_CASES if c[0] == "sum"]


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1) | (np.signbit(got) != np.signbit(want)).reshape(len(got), -1).any(axis=1))
    assert got.tobytes() == want.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"


def check_exact_transpose(pkg, rec, sp, what, fluid_only=False, moments_too=False):
    """Weight one, integer x and g: every sum is exact in any order, so adjoint_host(g) is A^T g of the integer matrix, bit for bit."""
    n = len(rec)
    for fac, c, self_, delta, moments in ((1.0, 3, False, False, False), (2.0, 5, True, False, False), (3.0, 2, False, True, False),
                                          (2.0, 4, True, True, False)) + (((1.0, 3, False, False, True), (2.0, 2, True, True, True)) if moments_too else ()):
        R = radius_of(sp, fac)
        kw = dict(self_=self_, fluid_only=fluid_only, delta=delta, moments=moments)
        A = AJ.dense(pkg, rec, sp, R, **kw)
        if not moments:
            assert (A == np.rint(A)).all()
            A = A.astype(np.int64)
        g = AJ.small_integers((n, 4, c) if moments else (n, c), 3 + c)
        want = AJ.transpose_apply(A, g)
        got = pkg.aggregate_adjoint_host(rec, sp, g, R, **kw)
        assert np.abs(want).max() < 2 ** 24 and np.abs(want).max() > 0
        same(got, (want + 0.0).astype(F), f"{what} {kw} R {fac} h")
        # ... and A itself is what the forward applies
        x = AJ.small_integers((n, c), 9 + c)
        fwd = pkg.aggregate_host(rec, sp, x, R, **kw)
        assert np.array_equal(fwd.reshape(n, -1, c).astype(np.float64), np.einsum("pik,kc->ipc", A.astype(np.float64), x.astype(np.float64))), what


def test_exact_transpose_uniform(pkg):
    check_exact_transpose(pkg, *QS.uniform(pkg, 1000, 21), "uniform")


def test_exact_transpose_lattice(pkg):
    check_exact_transpose(pkg, *QS.lattice(pkg), "lattice", moments_too=True)          # (multiples of 1/4: the moments are exact too)


def test_exact_transpose_coincident(pkg):
    rec, sp, same_ = QS.coincident(pkg)
    check_exact_transpose(pkg, rec, sp, "coincident")


@pytest.mark.parametrize("fluid_only", [False, True])
def test_exact_transpose_ghosts(pkg, fluid_only):
    rec, sp = QS.with_ghosts(pkg)
    check_exact_transpose(pkg, rec, sp, "ghosts", fluid_only=fluid_only)
    if fluid_only:
        g = AJ.small_integers((len(rec), 2), 1)
        out = pkg.aggregate_adjoint_host(rec, sp, g, radius_of(sp, 2.0), self_=True, fluid_only=True)
        ghost = rec["isGhost"] != 0
        assert not out[ghost].any() and not np.signbit(out[ghost]).any() and out[~ghost].any()


def test_exact_transpose_crowded_cell(pkg):
    rec, sp, start, members = QS.crowded_cell(pkg, 200)
    check_exact_transpose(pkg, rec, sp, "crowd 200")


def test_exact_transpose_query_cloud(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    gone = [5, 256, 700]
    for fac, c, fluid_only in ((1.0, 3, False), (2.0, 5, False), (3.0, 1, True)):
        R = radius_of(sp, fac)
        A = AJ.dense(pkg, rec, sp, R, points=pts, fluid_only=fluid_only).astype(np.int64)
        assert not A[0, gone].any() and A.any()
        g = AJ.small_integers((m, c), 5 + c)
        got = pkg.aggregate_adjoint_host(rec, sp, g, R, points=pts, fluid_only=fluid_only)
        same(got, (AJ.transpose_apply(A, g) + 0.0).astype(F), f"query cloud R {fac} h")
        g2 = g.copy()
        g2[gone] = 1000.0                                                               # what the non-finite points carry reaches nobody
        same(pkg.aggregate_adjoint_host(rec, sp, g2, R, points=pts, fluid_only=fluid_only), got, "non-finite points")
    lo, dims, cs = QS.grid(pkg, sp)
    outside = ((rec["pos"][:, :3] < lo) | (rec["pos"][:, :3] > lo + dims.astype(F) * cs)).any(axis=1)
    far = ((pts < lo) | (pts > lo + dims.astype(F) * cs)).any(axis=1)
    assert outside.any() and got[outside].any() and A[0][far].any()                     # particles and points in clamped cells take part


def test_identities_with_the_forward(pkg):
    """Particle targets without MOMENTS: the relation and the weights are symmetric, so the adjoint of g is the forward of g, byte for byte."""
    for rec, sp, what in ((*QS.uniform(pkg, 1000, 21), "uniform"), (*QS.with_ghosts(pkg), "ghosts")):
        for op, weight, self_, delta, moments, fac, c in SUM_CASES:
            if moments:
                continue
            for fluid_only in (False, True):
                g = values_for(len(rec), c, seed=31)
                R = radius_of(sp, fac)
                kw = dict(weight=weight, self_=self_, fluid_only=fluid_only, delta=delta)
                same(pkg.aggregate_adjoint_host(rec, sp, g, R, **kw), pkg.aggregate_host(rec, sp, g, R, **kw), f"{what} {kw}")
    rec, sp = QS.uniform(pkg, 300, 5)
    for self_ in (False, True):
        for delta in (False, True):
            for weight in ("one", "poly6"):
                g = values_for(len(rec), 5, seed=32)
                kw = dict(weight=weight, self_=self_, delta=delta)
                same(pkg.aggregate_adjoint_host(rec, sp, g, 1.0, **kw), pkg.aggregate_host(rec, sp, g, 1.0, **kw), str(kw))


def check_dot_product(pkg, rec, sp, case, what, points=None, fluid_only=False):
    op, weight, self_, delta, moments, fac, c = case
    rows = len(rec) if points is None else len(points)
    R = radius_of(sp, fac)
    kw = dict(weight=weight, fluid_only=fluid_only, moments=moments)
    if points is None:
        kw.update(self_=self_, delta=delta)
    x = values_for(len(rec), c, seed=41)
    g = np.random.default_rng(42 + c).normal(0.0, 1.0, (rows, 4, c) if moments else (rows, c)).astype(F)
    if points is not None:
        g[~np.isfinite(points).all(axis=1)] = 0.0
    y = pkg.aggregate_host(rec, sp, x, R, points=points, **kw)
    z = pkg.aggregate_adjoint_host(rec, sp, g, R, points=points, **kw)
    lhs = float((y.astype(np.float64) * g.astype(np.float64)).sum())
    rhs = float((x.astype(np.float64) * z.astype(np.float64)).sum())
    T, kmax = AJ.magnitudes(pkg, rec, sp, x, g, R, points=points, **kw)
    bound = AJ.dot_bound(T, kmax)
    print(f"{what} {kw} R {fac} h C {c}: <Ax, g> {lhs:.9g}, <x, A^T g> {rhs:.9g}, |difference| / bound {abs(lhs - rhs) / bound:.3g}, kmax {kmax}")
    assert T > 0 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("case", SUM_CASES + [("sum", "poly6", False, False, False, 2.0, 5), ("sum", "poly6", True, True, True, 1.0, 3)], ids=str)
def test_dot_product_particles(pkg, case):
    check_dot_product(pkg, *QS.uniform(pkg, 1000, 21), case, "uniform")
    check_dot_product(pkg, *QS.with_ghosts(pkg), case, "ghosts", fluid_only=True)


@pytest.mark.parametrize("case", SUM_QUERY_CASES, ids=str)
def test_dot_product_query(pkg, case):
    rec, sp, pts = QS.query_cloud(pkg)
    check_dot_product(pkg, rec, sp, case, "query cloud", points=pts)


def test_moments_adjoint_against_the_float64_transpose(pkg):
    """The MOMENTS contraction, the one particle-target case with device code of its own, row by row against A^T g in float64 within
    gamma_(4 k + 3) times the magnitudes (four terms per accepting row in one accumulator; three more roundings per term)."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    for delta, self_, weight in ((False, False, "one"), (True, False, "poly6"), (True, True, "one")):
        R = radius_of(sp, 2.0)
        kw = dict(weight=weight, self_=self_, delta=delta, moments=True)
        A = AJ.dense(pkg, rec, sp, R, **kw)
        g = np.random.default_rng(7).normal(0.0, 1.0, (len(rec), 4, 3)).astype(F)
        got = pkg.aggregate_adjoint_host(rec, sp, g, R, **kw).astype(np.float64)
        want = AJ.transpose_apply(A, g)
        mag, k = AJ.adjoint_magnitudes(pkg, rec, sp, g, R, **kw)
        bound = AR.gamma(4 * k.astype(np.float64) + 3)[:, None] * mag
        print(f"{kw}: max err / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3g}")
        assert (np.abs(got - want) <= bound).all()


def check_winners(pkg, rec, sp, x, what, points=None, fluid_only=False):
    n = len(rec)
    for op in ("max", "min"):
        for self_, delta, fac in ((False, False, 1.0), (True, False, 2.0), (False, True, 3.0), (True, True, 1.0)):
            if points is not None and (self_ or delta):
                continue
            R = radius_of(sp, fac)
            kw = dict(op=op, fluid_only=fluid_only) if points is not None else dict(op=op, self_=self_, fluid_only=fluid_only, delta=delta)
            out, cnt, arg = pkg.aggregate_arg_host(rec, sp, x, R, points=points, counts=True, **kw)
            plain, pcnt = pkg.aggregate_host(rec, sp, x, R, points=points, counts=True, **kw)
            assert out.tobytes() == plain.tobytes() and cnt.tobytes() == pcnt.tobytes(), (what, kw)
            want = AJ.winners(pkg, rec, sp, x, R, points=points, **kw)
            assert arg.dtype == np.int32 and np.array_equal(arg, want), (what, kw, np.argwhere(arg != want)[:5])
            # the winner holds the extremum: its reduced value has the key of out
            i, c = np.nonzero(arg >= 0)
            with np.errstate(invalid="ignore", over="ignore"):
                val = (x[arg[i, c], c] - x[i, c]).astype(F) if kw.get("delta") else x[arg[i, c], c]
            assert np.array_equal(AR.ordered(val), AR.ordered(out[i, c])), (what, kw)
            # routing integer-valued g through the winners is np.add.at
            g = AJ.small_integers(arg.shape, 17)
            got = pkg.aggregate_route_host(rec, sp, arg, g, R, points=points, **kw)
            same(got, (AJ.route(arg, g, n) + 0.0).astype(F), f"route {what} {kw}")


def test_winners_on_ties(pkg):
    """lattice and coincident: whole shells tie and only the id decides; values with few levels, so that ties are everywhere."""
    rec, sp = QS.lattice(pkg)
    x = np.random.default_rng(3).integers(0, 3, (len(rec), 5)).astype(F)
    check_winners(pkg, rec, sp, x, "lattice")
    rec, sp, same_ = QS.coincident(pkg)
    x = np.random.default_rng(4).integers(0, 2, (len(rec), 3)).astype(F)
    x[same_] = 7.0                                                                      # the eight coincident particles tie at the top
    check_winners(pkg, rec, sp, x, "coincident")
    arg = pkg.aggregate_arg_host(rec, sp, x, 1.0)[1]
    assert (arg[same_[1:]] == same_[0]).all() and (arg[same_[0]] == same_[1]).all()    # the smallest id among the others, never the own slot


def test_winners_with_nan_and_signed_zeros(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    x = values_for(len(rec), 4)
    x[::5, 0] = np.nan
    x[1::3, 1] = 0.0
    x[2::3, 1] = -0.0
    x[::3, 1] = np.nan
    x[:, 2] = np.nan                                                                    # a channel of NaNs: every arg is -1
    x[::2, 3] = -np.inf
    x[1::2, 3] = np.inf
    check_winners(pkg, rec, sp, x, "NaN, zeros, inf")
    out, arg = pkg.aggregate_arg_host(rec, sp, x, radius_of(sp, 2.0))
    assert (arg[:, 2] == -1).all() and np.isneginf(out[:, 2]).all()
    mx = pkg.aggregate_arg_host(rec, sp, x, radius_of(sp, 2.0), op="max")[1][:, 1]
    mn = pkg.aggregate_arg_host(rec, sp, x, radius_of(sp, 2.0), op="min")[1][:, 1]
    assert (mx[mx >= 0] % 3 != 0).all() and (mn[mn >= 0] % 3 != 0).all()                # a NaN never wins
    assert (mx % 3 == 1).sum() > 900 and (mn % 3 == 2).sum() > 900                      # +0 wins MAX, -0 wins MIN wherever the row has one
    rec, sp, pts = QS.query_cloud(pkg)
    xq = values_for(len(rec), 3)
    xq[::4, 1] = np.nan
    check_winners(pkg, rec, sp, xq, "query cloud", points=pts)
    assert (pkg.aggregate_arg_host(rec, sp, xq, 1.0, points=pts)[1][[5, 256, 700]] == -1).all()
    rec, sp = QS.with_ghosts(pkg)
    check_winners(pkg, rec, sp, values_for(len(rec), 2), "ghosts", fluid_only=True)


def test_tiny_scene_by_hand(pkg):
    """Three particles in a row, the middle one within R of both ends, the ends apart: every number can be checked by eye."""
    sp = QS.params(pkg)
    pos = np.array([[0.0, -0.5, 0.0], [0.4, -0.5, 0.0], [0.8, -0.5, 0.0]], F)
    rec = records(pkg, pos, np.zeros_like(pos))
    g = np.array([[1.0], [10.0], [100.0]], F)
    assert pkg.aggregate_adjoint_host(rec, sp, g, 0.5).tolist() == [[10.0], [101.0], [10.0]]
    assert pkg.aggregate_adjoint_host(rec, sp, g, 0.5, self_=True).tolist() == [[11.0], [111.0], [110.0]]
    assert pkg.aggregate_adjoint_host(rec, sp, g, 0.5, delta=True).tolist() == [[9.0], [81.0], [-90.0]]
    gm = np.zeros((3, 4, 1), F)
    gm[:, 1, 0] = [1.0, 10.0, 100.0]                                                    # the x moment: d_x = x_k - x_i
    got = pkg.aggregate_adjoint_host(rec, sp, gm, 0.5, moments=True)
    want = np.array([[(F(0.0) - F(0.4)) * F(10.0)], [F(0.4) * F(1.0) + (F(0.4) - F(0.8)) * F(100.0)], [(F(0.8) - F(0.4)) * F(10.0)]], F)
    assert np.array_equal(got, want)
    pts = np.array([[0.2, -0.5, 0.0], [np.nan, 0.0, 0.0], [0.2, -0.5, 0.0]], F)
    pv = np.array([[1.0], [5.0], [2.0]], F)
    assert pkg.aggregate_adjoint_host(rec, sp, pv, 0.3, points=pts).tolist() == [[3.0], [3.0], [0.0]]
    assert pkg.aggregate_adjoint_host(rec, sp, np.zeros((0, 1), F), 0.3, points=np.zeros((0, 3), F)).tolist() == [[0.0], [0.0], [0.0]]   # m = 0


def test_refusals_write_nothing(pkg):
    L = pkg.load_library()
    rec, sp = QS.uniform(pkg, 50, 3)
    n, h = len(rec), sp.param_h
    g = values_for(n, 4)
    g4 = np.zeros((n, 4, 4), F)
    arg = np.zeros((n, 4), np.int32)
    pts = np.zeros((3, 4), F)
    buf = np.full(n * 4 + 64, 7.0, F)
    out = buf[32:32 + n * 4]
    SUM, MAX = pkg.SPH_AGGREGATE_SUM, pkg.SPH_AGGREGATE_MAX
    p = lambda a: None if a is None else a.ctypes.data_as(vp)

    def adjoint(cfg, points=None, m=0, g_=g, out_=out, params=sp, cfg_null=False):
        rc = L.sph_aggregate_adjoint_host(p(rec), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg), p(points), m, p(g_), p(out_))
        assert (buf == 7.0).all()
        return rc

    def route(cfg, points=None, m=0, arg_=arg, g_=g, out_=out):
        rc = L.sph_aggregate_route_host(p(rec), n, C.byref(sp), C.byref(cfg), p(points), m, p(arg_), p(g_), p(out_))
        assert (buf == 7.0).all()
        return rc

    good = dict(radius=h, channels=4)
    assert adjoint(pkg.aggregate_config(**good), cfg_null=True) == -1 and adjoint(pkg.aggregate_config(**good), params=None) == -1
    assert adjoint(pkg.aggregate_config(**good), g_=None) == -1 and adjoint(pkg.aggregate_config(**good), out_=None) == -1
    for op in (pkg.SPH_AGGREGATE_MEAN, MAX, pkg.SPH_AGGREGATE_MIN, -1, 4):
        assert adjoint(pkg.aggregate_config(op=op, **good)) == -1, op
    assert b"SUM" in L.sph_last_error() or b"op" in L.sph_last_error()
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
        assert adjoint(pkg.aggregate_config(radius=R, channels=4)) == -1
    for bad in (dict(weight=-1), dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129), dict(channels=-3)):
        assert adjoint(pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    padded = pkg.aggregate_config(**good)
    padded.pad[1] = 1
    assert adjoint(padded) == -1
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):                      # particle targets only
        assert adjoint(pkg.aggregate_config(flags=flag, **good), points=pts, m=3) == -1
    assert adjoint(pkg.aggregate_config(**good), points=pts, m=1 << 31) == -1
    # out overlapping g, or the points, as address ranges
    both = np.full(n * 4 + 8, 7.0, F)
    assert L.sph_aggregate_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(**good)), None, 0, p(both[:n * 4]), p(both[8:])) == -1
    assert (both == 7.0).all() and b"overlap" in L.sph_last_error()
    big = np.full(n * 4 + 16, 7.0, F)
    assert L.sph_aggregate_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(**good)), p(big[n * 4 - 4:]), 3, p(g), p(big[:n * 4])) == -1
    assert (big == 7.0).all()
    # the routing: MAX / MIN only, a null arg, out overlapping arg
    assert route(pkg.aggregate_config(op=SUM, **good)) == -1 and route(pkg.aggregate_config(op=MAX, **good), arg_=None) == -1
    assert route(pkg.aggregate_config(op=MAX, **good), g_=None) == -1 and route(pkg.aggregate_config(op=MAX, **good), out_=None) == -1
    assert route(pkg.aggregate_config(op=MAX, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6, **good)) == -1
    mixed = np.full(n * 4 + 8, 7.0, F)
    assert L.sph_aggregate_route_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(op=MAX, **good)), None, 0, p(mixed[:n * 4].view(np.int32)), p(g),
                                      p(mixed[8:])) == -1 and (mixed == 7.0).all()
    # the winners: MAX / MIN only, a null arg
    o2, c2, a2 = np.full((n, 4), 7.0, F), np.full(n, 9, np.uint32), np.full((n, 4), 5, np.int32)

    def winners(cfg, arg_=a2):
        rc = L.sph_aggregate_arg_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(g), p(o2), p(c2), p(arg_))
        assert (o2 == 7.0).all() and (c2 == 9).all() and (a2 == 5).all()
        return rc

    assert winners(pkg.aggregate_config(op=SUM, **good)) == -1 and winners(pkg.aggregate_config(op=pkg.SPH_AGGREGATE_MEAN, **good)) == -1
    assert winners(pkg.aggregate_config(op=MAX, **good), arg_=None) == -1
    assert L.sph_aggregate_arg_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(op=MAX, **good)), None, 0, p(g), p(o2), p(c2), p(o2.view(np.int32))) == -1
    assert (o2 == 7.0).all()
    with pytest.raises(pkg.SphError):
        pkg.aggregate_adjoint_host(rec, sp, g[:-1], h)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_adjoint_host(rec, sp, g, h, moments=True)                         # (n, C) where (n, 4, C) is due
    with pytest.raises(pkg.SphError):
        pkg.aggregate_route_host(rec, sp, arg[:, :2], g, h)
    # the valid calls write every row and nothing else; m = 0 zeroes out; n = 0 succeeds and writes nothing
    assert L.sph_aggregate_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(**good)), None, 0, p(g), p(out)) == 0
    assert (buf[:32] == 7.0).all() and (buf[32 + n * 4:] == 7.0).all() and (out != 7.0).all()
    same(out.reshape(n, 4).copy(), pkg.aggregate_host(rec, sp, g, h), "the valid call")
    out[:] = 7.0
    assert L.sph_aggregate_adjoint_host(p(rec), n, C.byref(sp), C.byref(pkg.aggregate_config(flags=pkg.SPH_AGGREGATE_MOMENTS, **good)), p(pts), 0, p(g4), p(out)) == 0
    assert (out == 0.0).all() and not np.signbit(out).any() and (buf[:32] == 7.0).all() and (buf[32 + n * 4:] == 7.0).all()
    out[:] = 7.0
    assert L.sph_aggregate_adjoint_host(None, 0, C.byref(sp), C.byref(pkg.aggregate_config(**good)), p(pts), 3, p(g), p(out)) == 0 and (buf == 7.0).all()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    assert pkg.aggregate_adjoint_host(none, sp, np.zeros((5, 4), F), h, points=np.zeros((5, 3), F)).shape == (0, 4)
    assert pkg.aggregate_arg_host(none, sp, np.zeros((0, 2), F), h)[1].shape == (0, 2)
