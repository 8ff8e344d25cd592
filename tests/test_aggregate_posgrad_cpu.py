"""Position gradients of the neighbourhood sums on the CPU (the host twin of include/sph_abi.h "position gradients of the neighbourhood
sums"): the twin against the float64 definition within the bound derived in aggregate_posgrad_ref, the definition
against torch float64 autograd of a dense forward, the structure of the result, the refusals, the autograd layer on HostAggregateBackend
and the ABI table.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aggregate_posgrad_ref as PR
from aggregate_ref import radius_of, values_for
import query_scenes as QS
from support import records

F = np.float32
vp = C.c_void_p

# (weight, self_, delta, moments, radius in h, C): every flag combination the forward allows for a SUM, the three stencils and the
# channel counts 1, 5, 16, 33, 128 (a lone lane, a group tail, an exact fit, a partial second pass of no group, two channels per lane)
PARTICLE_CASES = [
    ("poly6", False, False, False, 1.0, 1),
    ("poly6", True, False, False, 2.0, 5),
    ("poly6", False, True, False, 3.0, 16),
    ("poly6", True, True, False, 1.0, 33),
    ("one", False, False, True, 2.0, 5),
    ("one", True, True, True, 1.0, 128),
    ("poly6", False, False, True, 3.0, 33),
    ("poly6", True, True, True, 2.0, 128),
    ("poly6", False, True, True, 1.0, 16),
    ("one", False, True, True, 3.0, 1),
    ("poly6", True, False, True, 1.0, 5),
    ("one", True, False, True, 3.0, 16),
]
QUERY_CASES = [("poly6", False, 1.0, 1), ("poly6", False, 2.0, 33), ("poly6", True, 3.0, 5), ("one", True, 2.0, 16), ("poly6", True, 1.0, 128), ("one", True, 3.0, 33)]


def grads_for(rows, c, moments, seed=61):
    return np.random.default_rng(seed + c).normal(0.0, 1.0, (rows, 4, c) if moments else (rows, c)).astype(F)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert got.tobytes() == want.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"


def plus_zero(a):
    return not a.any() and not np.signbit(a).any()


def within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"{what}: largest |gradient| {np.abs(want).max():.4g}, largest error {err.max():.3g}, largest error / bound {ratio:.3g}")
    assert np.abs(want).max() > 0 and (err <= bound).all(), what
    return ratio


# ---- the twin against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARTICLE_CASES, ids=str)
@pytest.mark.parametrize("fluid_only", [False, True])
def test_twin_against_definition_particles(pkg, case, fluid_only):
    weight, self_, delta, moments, fac, c = case
    rec, sp = QS.with_ghosts(pkg) if fluid_only else QS.uniform(pkg, 1000, 21)
    R = radius_of(sp, fac)
    x, g = values_for(len(rec), c, seed=51), grads_for(len(rec), c, moments)
    kw = dict(weight=weight, fluid_only=fluid_only, delta=delta, moments=moments)
    got = pkg.aggregate_position_grad_host(rec, sp, x, g, R, self_=self_, **kw)
    want, bound = PR.position_grad(pkg, rec, sp, x, g, R, **kw)
    within(got, want, bound, f"particles {kw} self {self_} R {fac} h C {c}")


@pytest.mark.parametrize("case", QUERY_CASES, ids=str)
@pytest.mark.parametrize("fluid_only", [False, True])
def test_twin_against_definition_query(pkg, case, fluid_only):
    weight, moments, fac, c = case
    rec, sp, pts = QS.query_cloud(pkg)
    if fluid_only:
        rec["isGhost"] = np.where(np.arange(len(rec)) % 3 == 0, 1, 0)
    R = radius_of(sp, fac)
    x, g = values_for(len(rec), c, seed=52), grads_for(len(pts), c, moments)
    kw = dict(weight=weight, fluid_only=fluid_only, moments=moments)
    gp, gx = pkg.aggregate_position_grad_host(rec, sp, x, g, R, points=pts, **kw)
    (wp, wx), (bp, bx) = PR.position_grad(pkg, rec, sp, x, g, R, points=pts, **kw)
    within(gp, wp, bp, f"query points {kw} R {fac} h C {c}")
    within(gx, wx, bx, f"query particles {kw} R {fac} h C {c}")
    assert plus_zero(gp[[5, 256, len(pts) - 1]])                                       # the non-finite points
    if fluid_only:
        assert plus_zero(gx[rec["isGhost"] != 0])


# ---- the definition against autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ["one", "poly6"])
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("moments", [False, True])
def test_definition_against_dense_autograd_particles(pkg, weight, delta, moments):
    rec, sp = QS.uniform(pkg, 200, 7)
    R = radius_of(sp, 2.0)
    x, g = values_for(200, 5, seed=53), grads_for(200, 5, moments)
    kw = dict(weight=weight, delta=delta, moments=moments)
    want, _, _ = PR.dense_autograd(pkg, rec, sp, x, g, R, **kw)
    ref, _ = PR.position_grad(pkg, rec, sp, x, g, R, **kw)
    scale = max(np.abs(want).max(), 1.0)
    print(f"{kw}: largest |gradient| {np.abs(want).max():.4g}, largest deviation {np.abs(ref - want).max():.3g}")
    assert np.abs(ref - want).max() <= 1e-11 * scale                                    # float64 rounding of some hundred terms
    assert (np.abs(want).max() > 0) == (weight == "poly6" or moments)


@pytest.mark.parametrize("weight", ["one", "poly6"])
@pytest.mark.parametrize("moments", [False, True])
def test_definition_against_dense_autograd_query(pkg, weight, moments):
    rec, sp = QS.uniform(pkg, 200, 7)
    pts = QS.box_cloud(np.random.default_rng(9), sp, 150)
    R = radius_of(sp, 2.0)
    x, g = values_for(200, 5, seed=54), grads_for(150, 5, moments)
    kw = dict(weight=weight, moments=moments)
    wx, wp, _ = PR.dense_autograd(pkg, rec, sp, x, g, R, points=pts, **kw)
    (rp, rx), _ = PR.position_grad(pkg, rec, sp, x, g, R, points=pts, **kw)
    scale = max(np.abs(wx).max(), np.abs(wp).max(), 1.0)
    assert np.abs(rx - wx).max() <= 1e-11 * scale and np.abs(rp - wp).max() <= 1e-11 * scale


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def test_one_without_moments_is_plus_zero(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    x = values_for(len(rec), 5)
    for delta in (False, True):
        assert plus_zero(pkg.aggregate_position_grad_host(rec, sp, x, grads_for(len(rec), 5, False), 1.0, weight="one", delta=delta, self_=True))
    gp, gx = pkg.aggregate_position_grad_host(rec, sp, x, grads_for(len(pts), 5, False), 1.0, points=pts, weight="one")
    assert plus_zero(gp) and plus_zero(gx) and gp.shape == (len(pts), 3) and gx.shape == (len(rec), 3)


def test_ghost_and_nonfinite_rows(pkg):
    rec, sp = QS.with_ghosts(pkg)
    x, g = values_for(len(rec), 5), grads_for(len(rec), 5, True)
    R = radius_of(sp, 2.0)
    ghost = rec["isGhost"] != 0
    out = pkg.aggregate_position_grad_host(rec, sp, x, g, R, weight="poly6", moments=True, fluid_only=True)
    assert plus_zero(out[ghost]) and (out[~ghost] != 0).any(axis=1).sum() > 500 and np.isfinite(out).all()
    # what a ghost carries reaches nobody
    x2, g2 = x.copy(), g.copy()
    x2[ghost], g2[ghost] = 1000.0, -1000.0
    same(pkg.aggregate_position_grad_host(rec, sp, x2, g2, R, weight="poly6", moments=True, fluid_only=True), out, "ghost payloads")
    # a non-finite particle: a +0 row, and nobody's candidate
    rec, sp = QS.uniform(pkg, 1000, 21)
    x, g = values_for(1000, 3), grads_for(1000, 3, True)
    bad = rec.copy()
    bad["pos"][7, 0], bad["pos"][500, 1], bad["pos"][999, 2] = np.nan, np.inf, -np.inf
    out = pkg.aggregate_position_grad_host(bad, sp, x, g, R, weight="poly6", moments=True, delta=True)
    assert plus_zero(out[[7, 500, 999]]) and np.isfinite(out).all()
    x2, g2 = x.copy(), g.copy()
    x2[[7, 500, 999]], g2[[7, 500, 999]] = 1e6, 1e6
    got = pkg.aggregate_position_grad_host(bad, sp, x2, g2, R, weight="poly6", moments=True, delta=True)
    keep = np.ones(1000, bool)
    keep[[7, 500, 999]] = False
    same(got[keep], out[keep], "non-finite particles' payloads")


def test_every_row_is_written_and_self_moves_nothing(pkg):
    L = pkg.load_library()
    rec, sp, pts = QS.query_cloud(pkg)
    n, m, c = len(rec), len(pts), 5
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    x, g, gq = values_for(n, c), grads_for(n, c, True), grads_for(m, c, True)
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    flags = pkg.SPH_AGGREGATE_MOMENTS
    cfg = pkg.aggregate_config(radius=1.0, channels=c, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6, flags=flags)
    for sentinel in (7.0, np.nan):
        buf = np.full(n * 3 + 64, sentinel, F)
        assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(x), p(g), None, p(buf[32:])) == 0
        inner = buf[32:32 + n * 3]
        edge = np.concatenate([buf[:32], buf[32 + n * 3:]])
        assert np.isfinite(inner).all() and ((edge == sentinel) | np.isnan(edge)).all()
        bq, bx = np.full(m * 3 + 64, sentinel, F), np.full(n * 3 + 64, sentinel, F)
        assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(p4), m, p(x), p(gq), p(bq[32:]), p(bx[32:])) == 0
        assert np.isfinite(bq[32:32 + m * 3]).all() and np.isfinite(bx[32:32 + n * 3]).all()
        for b, k in ((bq, m), (bx, n)):
            edge = np.concatenate([b[:32], b[32 + k * 3:]])
            assert ((edge == sentinel) | np.isnan(edge)).all()
    # one null output at a time gives the other's bytes
    both = pkg.aggregate_position_grad_host(rec, sp, x, gq, 1.0, points=pts, weight="poly6", moments=True)
    oq, ox = np.zeros((m, 3), F), np.zeros((n, 3), F)
    assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(p4), m, p(x), p(gq), p(oq), None) == 0
    assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(p4), m, p(x), p(gq), None, p(ox)) == 0
    same(oq, both[0], "points alone")
    same(ox, both[1], "particles alone")
    # SELF: the own slot's two terms are equal, so it is skipped
    for delta in (False, True):
        kw = dict(weight="poly6", moments=True, delta=delta)
        same(pkg.aggregate_position_grad_host(rec, sp, x, g, 1.0, self_=True, **kw), pkg.aggregate_position_grad_host(rec, sp, x, g, 1.0, self_=False, **kw), "SELF")


@pytest.mark.parametrize("moments", [False, True])
def test_net_gradient_within_the_bound(pkg, moments):
    """Translation invariance: every pair term enters twice with opposite signs, so the gradients sum to zero up to rounding."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    R = radius_of(sp, 2.0)
    x, g = values_for(1000, 5), grads_for(1000, 5, moments)
    kw = dict(weight="poly6", moments=moments, delta=True)
    out = pkg.aggregate_position_grad_host(rec, sp, x, g, R, **kw).astype(np.float64)
    _, bound = PR.position_grad(pkg, rec, sp, x, g, R, **kw)
    net, cap = np.abs(out.sum(axis=0)), bound.sum(axis=0)
    print(f"particles: |net| {net}, bound {cap}, largest row {np.abs(out).max():.4g}")
    assert (net <= cap).all() and np.abs(out).max() > 1e3 * net.max()
    rec, sp, pts = QS.query_cloud(pkg)
    x, g = values_for(len(rec), 5), grads_for(len(pts), 5, moments)
    kw = dict(weight="poly6", moments=moments)
    gp, gx = pkg.aggregate_position_grad_host(rec, sp, x, g, R, points=pts, **kw)
    _, (bp, bx) = PR.position_grad(pkg, rec, sp, x, g, R, points=pts, **kw)
    net = np.abs(gp.astype(np.float64).sum(axis=0) + gx.astype(np.float64).sum(axis=0))
    cap = bp.sum(axis=0) + bx.sum(axis=0)
    print(f"query: |net| {net}, bound {cap}")
    assert (net <= cap).all()


def test_coincident_and_lattice_are_finite_and_reproducible(pkg):
    for rec, sp, what in ((*QS.coincident(pkg)[:2], "coincident"), (*QS.lattice(pkg), "lattice")):
        n = len(rec)
        x, g = values_for(n, 5), grads_for(n, 5, True)
        R = radius_of(sp, 2.0)
        kw = dict(weight="poly6", moments=True, delta=True)
        a = pkg.aggregate_position_grad_host(rec, sp, x, g, R, **kw)
        b = pkg.aggregate_position_grad_host(rec.copy(), sp, x.copy(), g.copy(), R, **kw)
        assert np.isfinite(a).all() and a.any(), what
        same(a, b, what)
        want, bound = PR.position_grad(pkg, rec, sp, x, g, R, **kw)
        within(a, want, bound, what)


def test_tiny_scene_by_hand(pkg):
    """Two particles 0.25 apart on the x axis, one channel, POLY6 without MOMENTS, R = 0.5: L = g_0 w v_1 + g_1 w v_0 with
    w = (R2 - r2)^3, so dL/dx_1 = (g_0 v_1 + g_1 v_0) * (-6 t^2) * d_x = -dL/dx_0."""
    sp = QS.params(pkg)
    pos = np.array([[0.0, -0.5, 0.0], [0.25, -0.5, 0.0]], F)
    rec = records(pkg, pos, np.zeros_like(pos))
    x, g = np.array([[2.0], [3.0]], F), np.array([[5.0], [7.0]], F)
    t = F(0.25) - F(0.0625)
    w1 = F(-6.0) * (t * t)
    want1 = (w1 * F(14.0)) * F(0.25) - (w1 * F(15.0)) * F(-0.25)                       # e(0 -> 1) - e(1 -> 0): row 1
    out = pkg.aggregate_position_grad_host(rec, sp, x, g, 0.5, weight="poly6")
    assert out[1].tolist() == [float(F(want1)), 0.0, 0.0] and out[0].tolist() == [-float(F(want1)), 0.0, 0.0]
    assert out[1, 0] < 0                                                                 # moving apart lowers the weight
    gp, gx = pkg.aggregate_position_grad_host(rec, sp, x, np.array([[1.0]], F), 0.5, points=np.array([[0.0, -0.5, 0.0]], F), weight="poly6")
    assert gx[0].tolist() == [0.0, 0.0, 0.0] and gx[1, 0] == (w1 * F(3.0)) * F(0.25) and gp[0, 0] == -gx[1, 0]
    gp, gx = pkg.aggregate_position_grad_host(rec, sp, x, np.zeros((0, 1), F), 0.5, points=np.zeros((0, 3), F), weight="poly6")    # m = 0
    assert gp.shape == (0, 3) and plus_zero(gx)


def test_refusals_write_nothing(pkg):
    L = pkg.load_library()
    rec, sp = QS.uniform(pkg, 50, 3)
    n, h = len(rec), sp.param_h
    x, g = values_for(n, 4), grads_for(n, 4, False)
    pts = np.zeros((3, 4), F)
    gq = grads_for(3, 4, False)
    buf = np.full(n * 3 + 64, 7.0, F)
    out = buf[32:32 + n * 3]
    oq = np.full(9, 7.0, F)
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    POLY6 = pkg.SPH_AGGREGATE_WEIGHT_POLY6

    def call(cfg, points=None, m=0, x_=x, g_=g, outp=None, out_=out, params=sp, cfg_null=False):
        rc = L.sph_aggregate_posgrad_host(p(rec), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg), p(points), m, p(x_), p(g_),
                                          p(outp), p(out_))
        assert (buf == 7.0).all() and (oq == 7.0).all()
        return rc

    good = dict(radius=h, channels=4, weight=POLY6)
    assert call(pkg.aggregate_config(**good), cfg_null=True) == -1 and call(pkg.aggregate_config(**good), params=None) == -1
    assert call(pkg.aggregate_config(**good), x_=None) == -1 and call(pkg.aggregate_config(**good), g_=None) == -1
    assert call(pkg.aggregate_config(**good), out_=None) == -1
    for op in (pkg.SPH_AGGREGATE_MEAN, pkg.SPH_AGGREGATE_MAX, pkg.SPH_AGGREGATE_MIN, -1, 4):
        assert call(pkg.aggregate_config(op=op, **good)) == -1, op
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
        assert call(pkg.aggregate_config(radius=R, channels=4, weight=POLY6)) == -1
    for bad in (dict(weight=-1), dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129)):
        assert call(pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    padded = pkg.aggregate_config(**good)
    padded.pad[0] = 1
    assert call(padded) == -1
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):                      # particle targets only
        assert call(pkg.aggregate_config(flags=flag, **good), points=pts, m=3, g_=gq, outp=oq) == -1
    assert call(pkg.aggregate_config(**good), points=pts, m=1 << 31, g_=gq, outp=oq) == -1
    assert call(pkg.aggregate_config(**good), points=pts, m=3, g_=gq, outp=None, out_=None) == -1 and b"null" in L.sph_last_error()   # both outputs null
    # an output overlapping the values, g, or the other output
    cfg = pkg.aggregate_config(**good)
    both = np.full(n * 4 + 8, 7.0, F)
    assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(both[:n * 4]), p(g), None, p(both[8:])) == -1
    assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(x), p(both[:n * 4]), None, p(both[8:])) == -1
    assert (both == 7.0).all() and b"overlap" in L.sph_last_error()
    two = np.full(n * 3 + 4, 7.0, F)
    assert L.sph_aggregate_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(pts), 3, p(x), p(gq), p(two[:9]), p(two[4:])) == -1 and (two == 7.0).all()
    with pytest.raises(pkg.SphError):
        pkg.aggregate_position_grad_host(rec, sp, x, g[:-1], h)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_position_grad_host(rec, sp, x, g[:, :2], h)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_position_grad_host(rec, sp, x, g, h, moments=True)
    # n = 0: success, nothing is written
    assert L.sph_aggregate_posgrad_host(None, 0, C.byref(sp), C.byref(cfg), p(pts), 3, p(x), p(gq), p(oq), p(out)) == 0 and (buf == 7.0).all() and (oq == 7.0).all()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    assert pkg.aggregate_position_grad_host(none, sp, np.zeros((0, 2), F), np.zeros((0, 2), F), h).shape == (0, 3)


# ---- autograd on the host backend --------------------------------------------------------------------------------------------------------
def leaf(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F)).requires_grad_(True)


@pytest.mark.parametrize("op,weight,delta,moments", [("sum", "poly6", False, False), ("sum", "poly6", True, True), ("sum", "one", False, True),
                                                      ("mean", "poly6", False, False), ("mean", "poly6", True, False), ("mean", "one", True, False)])
def test_autograd_positions_against_dense_autograd(pkg, op, weight, delta, moments):
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    R = radius_of(sp, 2.0)
    be = pkg.HostAggregateBackend(rec, sp)
    x, pos = leaf(values_for(200, 5, seed=55)), be.positions().requires_grad_(True)
    kw = dict(op=op, weight=weight, self_=True, delta=delta, moments=moments)
    out = pkg.aggregate_autograd(be, None, x, R, positions=pos, **kw)
    same(out.detach().numpy(), pkg.aggregate_host(rec, sp, x.detach().numpy(), R, **kw), "the forward's bytes")
    g = grads_for(200, 5, moments)
    (out * torch.from_numpy(g)).sum().backward()
    want, _, dense_out = PR.dense_autograd(pkg, rec, sp, x.detach().numpy(), g, R, **kw)
    if op == "sum":
        _, bound = PR.position_grad(pkg, rec, sp, x.detach().numpy(), g, R, weight=weight, delta=delta, moments=moments)
    else:
        bound = PR.mean_bound(pkg, rec, sp, x.detach().numpy(), g, dense_out[:, 0, :], R, weight=weight, self_=True, delta=delta)
    if np.abs(want).max() > 0:
        within(pos.grad.numpy(), want, bound, f"autograd {kw}")
    else:
        assert plus_zero(pos.grad.numpy())
    assert x.grad is not None and x.grad.shape == x.shape


def test_autograd_points_grad_against_dense_autograd(pkg):
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    pts = QS.box_cloud(np.random.default_rng(9), sp, 150)
    R = radius_of(sp, 2.0)
    be = pkg.HostAggregateBackend(rec, sp)
    for op, moments in (("sum", True), ("mean", False)):
        x, pos, p = leaf(values_for(200, 5, seed=56)), be.positions().requires_grad_(True), leaf(pts)
        out = pkg.aggregate_autograd(be, p, x, R, op=op, weight="poly6", moments=moments, positions=pos, points_grad=True)
        same(out.detach().numpy(), pkg.aggregate_host(rec, sp, x.detach().numpy(), R, points=pts, op=op, weight="poly6", moments=moments), "the forward's bytes")
        g = grads_for(150, 5, moments)
        (out * torch.from_numpy(g)).sum().backward()
        wx, wp, dense_out = PR.dense_autograd(pkg, rec, sp, x.detach().numpy(), g, R, points=pts, weight="poly6", moments=moments, op=op)
        if op == "sum":
            _, (bp, bx) = PR.position_grad(pkg, rec, sp, x.detach().numpy(), g, R, points=pts, weight="poly6", moments=moments)
        else:
            bp, bx = PR.mean_bound(pkg, rec, sp, x.detach().numpy(), g, dense_out[:, 0, :], R, points=pts, weight="poly6")
        within(pos.grad.numpy(), wx, bx, f"{op}: positions")
        within(p.grad.numpy(), wp, bp, f"{op}: points")
    # points alone, as an (m, 4) tensor: the fourth column gets zeros
    x, p4 = leaf(values_for(200, 5, seed=56)), leaf(np.concatenate([pts, np.ones((150, 1), F)], axis=1))
    out = pkg.aggregate_autograd(be, p4, x, R, weight="poly6", points_grad=True)
    out.sum().backward()
    direct = pkg.aggregate_position_grad_host(rec, sp, x.detach().numpy(), np.ones((150, 5), F), R, points=pts, weight="poly6")[0]
    same(p4.grad.numpy()[:, :3].copy(), direct, "points alone")
    assert plus_zero(p4.grad.numpy()[:, 3])
    with pytest.raises(pkg.SphError):
        pkg.aggregate_autograd(be, pts, x, R, weight="poly6", points_grad=True)         # numpy points cannot receive a gradient


def test_autograd_max_gives_zeros_and_foreign_positions_raise(pkg):
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    be = pkg.HostAggregateBackend(rec, sp)
    x, pos = leaf(values_for(200, 3)), be.positions().requires_grad_(True)
    out = pkg.aggregate_autograd(be, None, x, 1.0, op="max", positions=pos)
    out.sum().backward()
    assert plus_zero(pos.grad.numpy()) and pos.grad.shape == (200, 3) and x.grad.sum() == out.numel()
    moved = be.positions()
    moved[17, 1] += 1e-3
    with pytest.raises(pkg.SphError, match="positions"):
        pkg.aggregate_autograd(be, None, x, 1.0, weight="poly6", positions=moved.requires_grad_(True))
    pkg.aggregate_autograd(be, None, x, 1.0, weight="poly6", positions=moved, check_state=False)      # (the check can be skipped)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_autograd(be, None, x, 1.0, positions=torch.zeros((200, 4)))


def test_autograd_defaults_are_the_existing_path(pkg):
    """positions None and points_grad False: the same Function, the same backend calls, the same bytes; a points tensor that requires
    grad still gets None."""
    torch = pytest.importorskip("torch")
    rec, sp, pts = QS.query_cloud(pkg)
    calls = []

    class Spy(pkg.HostAggregateBackend):
        def __getattribute__(self, name):
            if name in ("forward", "adjoint", "arg", "route", "posgrad", "positions"):
                calls.append(name)
            return super().__getattribute__(name)

    be = Spy(rec, sp)
    for op, weight in (("sum", "poly6"), ("mean", "poly6"), ("max", "one")):
        x = leaf(values_for(len(rec), 4))
        out = pkg.aggregate_autograd(be, None, x, 1.0, op=op, weight=weight, self_=True)
        assert type(out.grad_fn).__name__.startswith("AggregateFunction")
        g = torch.from_numpy(grads_for(len(rec), 4, False))
        (out * g).sum().backward()
        same(out.detach().numpy(), pkg.aggregate_host(rec, sp, x.detach().numpy(), 1.0, op=op, weight=weight, self_=True), op)
        if op == "sum":
            same(x.grad.numpy(), pkg.aggregate_adjoint_host(rec, sp, g.numpy(), 1.0, weight=weight, self_=True), "values.grad")
    assert "posgrad" not in calls and "positions" not in calls
    good = torch.from_numpy(np.where(np.isfinite(pts), pts, F(0))).requires_grad_(True)
    x = leaf(values_for(len(rec), 4))
    pkg.aggregate_autograd(be, good, x, 1.0, weight="poly6").sum().backward()
    assert good.grad is None and x.grad is not None and "posgrad" not in calls


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_header(pkg):
    import os
    from conftest import ROOT
    L = pkg.load_library()
    with open(os.path.join(ROOT, "include", "sph_abi.h")) as fh:
        text = fh.read()
    for name in ("sph_aggregate_posgrad_particles", "sph_aggregate_posgrad_query", "sph_aggregate_posgrad_staged", "sph_aggregate_posgrad_host"):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and f"int {name}(" in text, name
    assert "#define SPH_ABI_VERSION 4" in text and "sph_aggregate_posgrad_particles / _query / _staged / _host" in text
