"""Position gradients of the basis sums on the CPU (the host twin of include/sph_abi.h "position gradients of the basis sums"; DESIGN.md
section 3y): the twin against the float64 definition within the bound derived in conv_posgrad_ref (nothing excluded: the reference takes
its cells from the fp32 rule), the definition against torch float64 autograd of a dense forward, the structure of the result, the
refusals, continuous_conv's positions= / points_grad= on HostAggregateBackend and the ABI table.  No GPU.

The autograd bounds.  positions.grad of continuous_conv is a sum of basis_posgrad calls, one per block of input channels, each with the
upstream h_block = g' @ F_block^T, plus with normalize (poly6) the one-channel posgrad of ones (section 3x) with the upstream
-sum_o g'[i][o] out[i][o].  The bound is the sum of the calls' bounds, each for its upstream in float64; h_block is a torch fp32 matrix
product of Cout terms (and g' = g / W one division), so it is within gamma_(Cout + 1) |g'| @ |F_block^T| of the float64 one, and the
gradient moves by at most the call's magnitude sums for that perturbation (conv_posgrad_ref.position_grad(magnitudes=True)).  The
rounding of the W term's upstream is not added (as aggregate_posgrad_ref.mean_bound); the figures printed say how much is used."""
import ctypes as C

import numpy as np
import pytest

import aggregate_posgrad_ref as PR
import aggregate_ref as AR
from aggregate_ref import radius_of, values_for
import conv_posgrad_ref as GR
from conv_posgrad_ref import CASES
from conv_ref import planes_for, same
import query_scenes as QS

F = np.float32
vp = C.c_void_p


def plus_zero(a):
    return not a.any() and not np.signbit(a).any()


def within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"{what}: largest |gradient| {np.abs(want).max():.4g}, largest error {err.max():.3g}, largest error / bound {ratio:.3g}")
    assert np.abs(want).max() > 0 and (err <= bound).all(), what
    return ratio


# ---- the twin against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("fluid_only", [False, True])
def test_twin_against_definition_particles(pkg, case, fluid_only):
    K, weight, fac, c = case
    rec, sp = QS.with_ghosts(pkg) if fluid_only else QS.uniform(pkg, 1000, 21)
    R = radius_of(sp, fac)
    x, g = values_for(len(rec), c, seed=51), planes_for(len(rec), K, c)
    kw = dict(size=K, weight=weight, fluid_only=fluid_only)
    got = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, self_=bool(c & 1), **kw)
    want, bound = GR.position_grad(pkg, rec, sp, x, g, R, **kw)
    within(got, want, bound, f"particles {kw} R {fac} h C {c}")
    if fluid_only:
        assert plus_zero(got[rec["isGhost"] != 0])


@pytest.mark.parametrize("case", CASES[:6], ids=str)
@pytest.mark.parametrize("fluid_only", [False, True])
def test_twin_against_definition_query(pkg, case, fluid_only):
    K, weight, fac, c = case
    rec, sp, pts = QS.query_cloud(pkg)
    if fluid_only:
        rec["isGhost"] = np.where(np.arange(len(rec)) % 3 == 0, 1, 0)
    R = radius_of(sp, fac)
    x, g = values_for(len(rec), c, seed=52), planes_for(len(pts), K, c)
    kw = dict(size=K, weight=weight, fluid_only=fluid_only)
    gp, gx = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, points=pts, **kw)
    (wp, wx), (bp, bx) = GR.position_grad(pkg, rec, sp, x, g, R, points=pts, **kw)
    within(gp, wp, bp, f"query points {kw} R {fac} h C {c}")
    within(gx, wx, bx, f"query particles {kw} R {fac} h C {c}")
    assert plus_zero(gp[[5, 256, len(pts) - 1]])                                       # the non-finite points
    if fluid_only:
        assert plus_zero(gx[rec["isGhost"] != 0])


# ---- the definition against autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("weight", ["one", "poly6"])
@pytest.mark.parametrize("fluid_only", [False, True])
def test_definition_against_dense_autograd_particles(pkg, K, weight, fluid_only):
    rec, sp = QS.uniform(pkg, 200, 7)
    if fluid_only:
        rec["isGhost"] = np.where(np.arange(len(rec)) % 4 == 0, 1, 0)
    R = radius_of(sp, 2.0)
    x, g = values_for(200, 5, seed=53), planes_for(200, K, 5)
    kw = dict(size=K, weight=weight, fluid_only=fluid_only)
    want, _, _ = GR.dense_autograd(pkg, rec, sp, x, g, R, self_=True, **kw)
    ref, _ = GR.position_grad(pkg, rec, sp, x, g, R, **kw)
    scale = max(np.abs(want).max(), 1.0)
    print(f"{kw}: largest |gradient| {np.abs(want).max():.4g}, largest deviation {np.abs(ref - want).max():.3g}")
    assert np.abs(ref - want).max() <= 1e-11 * scale and np.abs(want).max() > 0        # float64 rounding of some thousand terms


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("weight", ["one", "poly6"])
def test_definition_against_dense_autograd_query(pkg, K, weight):
    rec, sp = QS.uniform(pkg, 200, 7)
    pts = QS.box_cloud(np.random.default_rng(9), sp, 150)
    R = radius_of(sp, 2.0)
    x, g = values_for(200, 5, seed=54), planes_for(150, K, 5)
    kw = dict(size=K, weight=weight, fluid_only=K == 3)
    if K == 3:
        rec["isGhost"] = np.where(np.arange(len(rec)) % 4 == 0, 1, 0)
    wx, wp, _ = GR.dense_autograd(pkg, rec, sp, x, g, R, points=pts, **kw)
    (rp, rx), _ = GR.position_grad(pkg, rec, sp, x, g, R, points=pts, **kw)
    scale = max(np.abs(wx).max(), np.abs(wp).max(), 1.0)
    print(f"{kw}: largest |gradient| {scale:.4g}, largest deviation {max(np.abs(rx - wx).max(), np.abs(rp - wp).max()):.3g}")
    assert np.abs(rx - wx).max() <= 1e-11 * scale and np.abs(rp - wp).max() <= 1e-11 * scale and np.abs(wp).max() > 0


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ["one", "poly6"])
def test_column_sums_vanish_within_the_bound(pkg, weight):
    """Translation invariance: every pair term enters twice with opposite signs, so the gradients sum to zero up to rounding."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    R = radius_of(sp, 2.0)
    x, g = values_for(1000, 5), planes_for(1000, 3, 5)
    out = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, size=3, weight=weight).astype(np.float64)
    _, bound = GR.position_grad(pkg, rec, sp, x, g, R, size=3, weight=weight)
    net, cap = np.abs(out.sum(axis=0)), bound.sum(axis=0)
    print(f"particles {weight}: |column sums| {net}, bound {cap}, largest row {np.abs(out).max():.4g}")
    assert (net <= cap).all() and np.abs(out).max() > 1e3 * net.max()
    rec, sp, pts = QS.query_cloud(pkg)
    x, g = values_for(len(rec), 5), planes_for(len(pts), 3, 5)
    gp, gx = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, points=pts, size=3, weight=weight)
    _, (bp, bx) = GR.position_grad(pkg, rec, sp, x, g, R, points=pts, size=3, weight=weight)
    net = np.abs(gp.astype(np.float64).sum(axis=0) + gx.astype(np.float64).sum(axis=0))
    print(f"query {weight}: |column sums| {net}, bound {bp.sum(axis=0) + bx.sum(axis=0)}")
    assert (net <= bp.sum(axis=0) + bx.sum(axis=0)).all()


def test_self_moves_no_byte_and_one_is_not_zero(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    x, g = values_for(1000, 3), planes_for(1000, 4, 3)
    for weight in ("one", "poly6"):
        a = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, 1.0, weight=weight, self_=False)
        same(pkg.aggregate_basis_position_grad_host(rec, sp, x, g, 1.0, weight=weight, self_=True), a, "SELF " + weight)
        assert (a != 0).any(axis=1).sum() > 900 and np.isfinite(a).all(), weight        # weight "one": the hats still move


def test_ghost_and_nonfinite_rows(pkg):
    rec, sp = QS.with_ghosts(pkg)
    x, g = values_for(len(rec), 5), planes_for(len(rec), 3, 5)
    R = radius_of(sp, 2.0)
    ghost = rec["isGhost"] != 0
    out = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, size=3, fluid_only=True)
    assert plus_zero(out[ghost]) and (out[~ghost] != 0).any(axis=1).sum() > 500 and np.isfinite(out).all()
    x2, g2 = x.copy(), g.copy()                                                         # what a ghost carries reaches nobody
    x2[ghost], g2[ghost] = 1000.0, -1000.0
    same(pkg.aggregate_basis_position_grad_host(rec, sp, x2, g2, R, size=3, fluid_only=True), out, "ghost payloads")
    rec, sp = QS.uniform(pkg, 1000, 21)                                                 # a non-finite particle: a +0 row, nobody's candidate
    x, g = values_for(1000, 3), planes_for(1000, 4, 3)
    bad = rec.copy()
    bad["pos"][7, 0], bad["pos"][500, 1], bad["pos"][999, 2] = np.nan, np.inf, -np.inf
    out = pkg.aggregate_basis_position_grad_host(bad, sp, x, g, R)
    assert plus_zero(out[[7, 500, 999]]) and np.isfinite(out).all()
    x2, g2 = x.copy(), g.copy()
    x2[[7, 500, 999]], g2[[7, 500, 999]] = 1e6, 1e6
    keep = np.ones(1000, bool)
    keep[[7, 500, 999]] = False
    same(pkg.aggregate_basis_position_grad_host(bad, sp, x2, g2, R)[keep], out[keep], "non-finite particles' payloads")
    pts = QS.query_cloud(pkg)[2]
    gp, gx = pkg.aggregate_basis_position_grad_host(bad, sp, x, planes_for(len(pts), 4, 3), R, points=pts)
    assert plus_zero(gp[[5, 256, len(pts) - 1]]) and plus_zero(gx[[7, 500, 999]]) and np.isfinite(gp).all() and np.isfinite(gx).all()


def test_every_row_is_written_and_one_null_output_gives_the_pair_bytes(pkg):
    L = pkg.load_library()
    rec, sp, pts = QS.query_cloud(pkg)
    n, m, c, K = len(rec), len(pts), 5, 3
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    x, g, gq = values_for(n, c), planes_for(n, K, c), planes_for(m, K, c)
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    cfg = pkg.basis_config(radius=1.0, channels=c, size=K)
    for sentinel in (7.0, np.nan):
        buf = np.full(n * 3 + 64, sentinel, F)
        assert L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(x), p(g), None, p(buf[32:])) == 0
        edge = np.concatenate([buf[:32], buf[32 + n * 3:]])
        assert np.isfinite(buf[32:32 + n * 3]).all() and ((edge == sentinel) | np.isnan(edge)).all()
        bq, bx = np.full(m * 3 + 64, sentinel, F), np.full(n * 3 + 64, sentinel, F)
        assert L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(p4), m, p(x), p(gq), p(bq[32:]), p(bx[32:])) == 0
        assert np.isfinite(bq[32:32 + m * 3]).all() and np.isfinite(bx[32:32 + n * 3]).all()
        for b, k in ((bq, m), (bx, n)):
            edge = np.concatenate([b[:32], b[32 + k * 3:]])
            assert ((edge == sentinel) | np.isnan(edge)).all()
    both = pkg.aggregate_basis_position_grad_host(rec, sp, x, gq, 1.0, points=pts, size=K)
    a = pkg.aggregate_basis_position_grad_host(rec, sp, x, gq, 1.0, points=pts, size=K, want_particles=False)
    b = pkg.aggregate_basis_position_grad_host(rec, sp, x, gq, 1.0, points=pts, size=K, want_points=False)
    assert a[1] is None and b[0] is None
    same(a[0], both[0], "points alone"), same(b[1], both[1], "particles alone")
    gp, gx = pkg.aggregate_basis_position_grad_host(rec, sp, x, np.zeros((0, K ** 3, c), F), 1.0, points=np.zeros((0, 3), F), size=K)     # m = 0
    assert gp.shape == (0, 3) and plus_zero(gx) and gx.shape == (n, 3)


def test_coincident_and_lattice_are_finite_and_reproducible(pkg):
    for rec, sp, what in ((*QS.coincident(pkg)[:2], "coincident"), (*QS.lattice(pkg), "lattice")):
        n = len(rec)
        x, g = values_for(n, 5), planes_for(n, 4, 5)
        R = radius_of(sp, 2.0)
        a = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R)
        b = pkg.aggregate_basis_position_grad_host(rec.copy(), sp, x.copy(), g.copy(), R)
        assert np.isfinite(a).all() and a.any(), what
        same(a, b, what)
        within(a, *GR.position_grad(pkg, rec, sp, x, g, R), what)


def test_refusals_write_nothing(pkg):
    L = pkg.load_library()
    rec, sp = QS.uniform(pkg, 50, 3)
    n, h, K, c = len(rec), sp.param_h, 2, 4
    x, g = values_for(n, c), planes_for(n, K, c)
    pts = np.zeros((3, 4), F)
    gq = planes_for(3, K, c)
    buf = np.full(n * 3 + 64, 7.0, F)
    out = buf[32:32 + n * 3]
    oq = np.full(9, 7.0, F)
    p = lambda a: None if a is None else a.ctypes.data_as(vp)

    def call(cfg, points=None, m=0, x_=x, g_=g, outp=None, out_=out, params=sp, cfg_null=False):
        rc = L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg), p(points), m, p(x_),
                                                p(g_), p(outp), p(out_))
        assert (buf == 7.0).all() and (oq == 7.0).all()
        return rc

    good = dict(radius=h, channels=c, size=K)
    assert call(pkg.basis_config(**good), cfg_null=True) == -1 and call(pkg.basis_config(**good), params=None) == -1
    assert call(pkg.basis_config(**good), x_=None) == -1 and call(pkg.basis_config(**good), g_=None) == -1
    assert call(pkg.basis_config(**good), out_=None) == -1
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
        assert call(pkg.basis_config(**dict(good, radius=R))) == -1
    for bad in (dict(weight=-1), dict(weight=2), dict(flags=4), dict(flags=8), dict(flags=16), dict(channels=0), dict(channels=129), dict(kind=1), dict(size=1),
                dict(size=5)):
        assert call(pkg.basis_config(**dict(good, **bad))) == -1, bad
    padded = pkg.basis_config(**good)
    padded.pad[0] = 1
    assert call(padded) == -1
    assert call(pkg.basis_config(flags=pkg.SPH_AGGREGATE_SELF, **good), points=pts, m=3, g_=gq, outp=oq) == -1       # particle targets only
    assert call(pkg.basis_config(**good), points=pts, m=1 << 31, g_=gq, outp=oq) == -1
    assert call(pkg.basis_config(**good), points=pts, m=3, g_=gq, outp=None, out_=None) == -1 and b"null" in L.sph_last_error()   # both outputs null
    cfg = pkg.basis_config(**good)                                                      # an output overlapping the values, g, or the other output
    both = np.full(n * c * K ** 3 + 8, 7.0, F)
    assert L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(both[:n * c]), p(g), None, p(both[8:])) == -1
    assert L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), None, 0, p(x), p(both[:n * c * K ** 3]), None, p(both[8:])) == -1
    assert (both == 7.0).all() and b"overlap" in L.sph_last_error()
    two = np.full(n * 3 + 4, 7.0, F)
    assert L.sph_aggregate_basis_posgrad_host(p(rec), n, C.byref(sp), C.byref(cfg), p(pts), 3, p(x), p(gq), p(two[:9]), p(two[4:])) == -1 and (two == 7.0).all()
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_position_grad_host(rec, sp, x, g[:-1], h, size=K)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_position_grad_host(rec, sp, x, g[:, :, :2], h, size=K)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_basis_position_grad_host(rec, sp, x, g, h, size=3)
    # n = 0: success, nothing is written
    assert L.sph_aggregate_basis_posgrad_host(None, 0, C.byref(sp), C.byref(cfg), p(pts), 3, p(x), p(gq), p(oq), p(out)) == 0 and (buf == 7.0).all() and (oq == 7.0).all()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    assert pkg.aggregate_basis_position_grad_host(none, sp, np.zeros((0, 2), F), np.zeros((0, 8, 2), F), h, size=2).shape == (0, 3)


# ---- autograd on the host backend --------------------------------------------------------------------------------------------------------
def leaf(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F)).requires_grad_(True)


def filters_for(K, cin, cout, seed=81):
    return np.random.default_rng(seed + K + cin).normal(0.0, 0.5, (K, K, K, cin, cout)).astype(F)


def conv_bound(pkg, rec, sp, x, g, out64, filters, R, blocks, points=None, weight="poly6", self_=False, normalize=False):
    """The summed bounds of the module docstring: (boundPoints or None, boundParticles)."""
    n, K, cout = len(rec), filters.shape[0], filters.shape[4]
    g64 = np.asarray(g, np.float64)
    if normalize:
        W = pkg.aggregate_host(rec, sp, np.ones((n, 1), F), R, points=points, weight=weight, self_=self_).astype(np.float64).reshape(-1)
        g64 = np.where(W[:, None] != 0, g64 / np.where(W != 0, W, 1.0)[:, None], 0.0)
    tot = None
    add = lambda t, b: b if t is None else (t + b if points is None else (t[0] + b[0], t[1] + b[1]))
    for c0, c1 in blocks:
        Fb = filters[:, :, :, c0:c1, :].astype(np.float64).reshape(-1, cout)
        h = (g64 @ Fb.T).reshape(len(g64), K ** 3, c1 - c0)
        dh = AR.gamma(cout + 1.0) * (np.abs(g64) @ np.abs(Fb).T).reshape(h.shape)
        tot = add(tot, GR.position_grad(pkg, rec, sp, x[:, c0:c1], h, R, points=points, size=K, weight=weight)[1])
        tot = add(tot, GR.position_grad(pkg, rec, sp, x[:, c0:c1], dh, R, points=points, size=K, weight=weight, magnitudes=True)[2])
    if normalize and weight != "one":
        up = -(g64 * out64).sum(axis=1, keepdims=True)
        tot = add(tot, PR.position_grad(pkg, rec, sp, np.ones((n, 1), F), up, R, points=points, weight=weight)[1])
    return (None, tot) if points is None else tot


def test_autograd_one_block_is_the_host_call(pkg):
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    R = radius_of(sp, 2.0)
    be = pkg.HostAggregateBackend(rec, sp)
    for K, weight, self_ in ((4, "poly6", True), (3, "one", False)):
        x, flt, pos = leaf(values_for(200, 5, seed=55)), leaf(filters_for(K, 5, 3)), be.positions().requires_grad_(True)
        out = pkg.continuous_conv(be, None, x, flt, R, weight=weight, self_=self_, positions=pos)
        g = torch.from_numpy(values_for(200, 3, seed=57))
        (out * g).sum().backward()
        h = (g @ flt.detach().reshape(-1, 3).t()).reshape(200, K ** 3, 5).contiguous().numpy()
        same(pos.grad.numpy(), pkg.aggregate_basis_position_grad_host(rec, sp, x.detach().numpy(), h, R, size=K, weight=weight, self_=self_), f"positions.grad {K} {weight}")
        # x.grad and filters.grad: the bytes of a call without the keyword
        x2, flt2 = leaf(x.detach().numpy()), leaf(flt.detach().numpy())
        out2 = pkg.continuous_conv(be, None, x2, flt2, R, weight=weight, self_=self_)
        (out2 * g).sum().backward()
        same(out.detach().numpy(), out2.detach().numpy(), "out"), same(x.grad.numpy(), x2.grad.numpy(), "x.grad"), same(flt.grad.numpy(), flt2.grad.numpy(), "filters.grad")
        assert type(out.grad_fn).__name__.startswith("ContinuousConvPositionFunction") and type(out2.grad_fn).__name__.startswith("ContinuousConvFunction")


@pytest.mark.parametrize("weight,normalize,small", [("poly6", True, False), ("poly6", False, True), ("poly6", True, True), ("one", True, True)])
def test_autograd_positions_against_dense_autograd(pkg, weight, normalize, small):
    torch = pytest.importorskip("torch")
    from importlib import import_module
    rec, sp = QS.uniform(pkg, 200, 7)
    R = radius_of(sp, 2.0)
    K, cin, cout = 3, 5, 4
    be = pkg.HostAggregateBackend(rec, sp)
    x, flt, pos = leaf(values_for(200, cin, seed=55)), leaf(filters_for(K, cin, cout)), be.positions().requires_grad_(True)
    max_bytes = 200 * K ** 3 * 4 * 3 if small else 2 ** 31                              # blocks of 3 and 2 channels
    blocks = import_module(pkg.__name__ + ".autograd")._conv_blocks(200, K ** 3, cin, max_bytes)
    assert len(blocks) == (2 if small else 1)
    out = pkg.continuous_conv(be, None, x, flt, R, weight=weight, self_=True, normalize=normalize, positions=pos, max_basis_bytes=max_bytes)
    g = values_for(200, cout, seed=58)
    (out * torch.from_numpy(g)).sum().backward()
    xn, fn = x.detach().numpy(), flt.detach().numpy()
    want, _, out64 = GR.dense_autograd(pkg, rec, sp, xn, g, R, size=K, weight=weight, self_=True, filters=fn, normalize=normalize)
    _, bound = conv_bound(pkg, rec, sp, xn, g, out64, fn, R, blocks, weight=weight, self_=True, normalize=normalize)
    within(pos.grad.numpy(), want, bound, f"continuous_conv {weight} normalize {normalize} blocks {len(blocks)}")
    assert x.grad is not None and flt.grad is not None


def test_autograd_points_grad(pkg):
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    pts = QS.box_cloud(np.random.default_rng(9), sp, 150)
    R = radius_of(sp, 2.0)
    K, cin, cout = 4, 3, 2
    be = pkg.HostAggregateBackend(rec, sp)
    for normalize in (False, True):
        x, flt, pos, p = leaf(values_for(200, cin, seed=56)), leaf(filters_for(K, cin, cout)), be.positions().requires_grad_(True), leaf(pts)
        out = pkg.continuous_conv(be, p, x, flt, R, self_=False, normalize=normalize, positions=pos, points_grad=True)
        g = values_for(150, cout, seed=59)
        (out * torch.from_numpy(g)).sum().backward()
        xn, fn = x.detach().numpy(), flt.detach().numpy()
        wx, wp, out64 = GR.dense_autograd(pkg, rec, sp, xn, g, R, points=pts, size=K, filters=fn, normalize=normalize)
        bp, bx = conv_bound(pkg, rec, sp, xn, g, out64, fn, R, [(0, cin)], points=pts, normalize=normalize)
        within(pos.grad.numpy(), wx, bx, f"normalize {normalize}: positions")
        within(p.grad.numpy(), wp, bp, f"normalize {normalize}: points")
        if not normalize:
            h = (torch.from_numpy(g) @ flt.detach().reshape(-1, cout).t()).reshape(150, K ** 3, cin).contiguous().numpy()
            direct = pkg.aggregate_basis_position_grad_host(rec, sp, xn, h, R, points=pts, size=K)
            same(p.grad.numpy(), direct[0], "points.grad"), same(pos.grad.numpy(), direct[1], "positions.grad")
    # points alone, as an (m, 4) tensor: the fourth column gets zeros, and the particles' walk is not asked for
    calls = []

    class Spy(pkg.HostAggregateBackend):
        def basis_posgrad(self, *a, **kw):
            calls.append(a[-2:])
            return super().basis_posgrad(*a, **kw)

    x, flt, p4 = leaf(values_for(200, cin, seed=56)), leaf(filters_for(K, cin, cout)), leaf(np.concatenate([pts, np.ones((150, 1), F)], axis=1))
    pkg.continuous_conv(Spy(rec, sp), p4, x, flt, R, self_=False, points_grad=True).sum().backward()
    assert calls == [(True, False)] and plus_zero(p4.grad.numpy()[:, 3]) and p4.grad.numpy()[:, :3].any()
    with pytest.raises(pkg.SphError):
        pkg.continuous_conv(be, pts, x, flt, R, self_=False, points_grad=True)          # numpy points cannot receive a gradient


def test_autograd_defaults_are_the_existing_path_and_foreign_positions_raise(pkg):
    """positions None and points_grad False: the same Function, the same backend calls in the same sequence; a positions tensor that
    differs raises."""
    torch = pytest.importorskip("torch")
    rec, sp = QS.uniform(pkg, 200, 7)
    calls = []

    class Spy(pkg.HostAggregateBackend):
        def __getattribute__(self, name):
            if name in ("forward", "adjoint", "posgrad", "positions", "basis", "basis_adjoint", "basis_posgrad", "state"):
                calls.append(name)
            return super().__getattribute__(name)

    be = Spy(rec, sp)
    x, flt = leaf(values_for(200, 5)), leaf(filters_for(3, 5, 2))
    first = pkg.continuous_conv(be, None, x, flt, 1.0, normalize=True, max_basis_bytes=200 * 27 * 4 * 3)
    second = pkg.continuous_conv(be, None, x, flt, 1.0)
    assert type(first.grad_fn) is type(second.grad_fn) and type(first.grad_fn).__name__.startswith("ContinuousConvFunction")
    first.sum().backward()
    # two blocks, normalize: state, basis x 2, forward (W); backward: state, per block basis (filters) and basis_adjoint (x)
    assert calls == ["state", "basis", "basis", "forward", "state", "basis", "state", "basis", "basis_adjoint", "basis", "basis_adjoint"], calls
    del calls[:]
    pos = be.positions().requires_grad_(True)
    third = pkg.continuous_conv(be, None, x, flt, 1.0, normalize=True, positions=pos)
    third.sum().backward()
    assert calls == ["positions", "positions", "state", "basis", "forward", "state", "basis", "basis_adjoint", "basis_posgrad", "posgrad"], calls
    moved = be.positions()
    moved[17, 1] += 1e-3
    with pytest.raises(pkg.SphError, match="positions"):
        pkg.continuous_conv(be, None, x, flt, 1.0, positions=moved.requires_grad_(True))
    pkg.continuous_conv(be, None, x, flt, 1.0, positions=moved, check_state=False)      # (the check can be skipped)
    with pytest.raises(pkg.SphError):
        pkg.continuous_conv(be, None, x, flt, 1.0, positions=torch.zeros((200, 4)))
    with pytest.raises(RuntimeError):                                                   # once differentiable
        y = pkg.continuous_conv(be, None, x, flt, 1.0, positions=pos)
        (gx,) = torch.autograd.grad(y.sum(), pos, create_graph=True)
        gx.sum().backward()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_table_and_header(pkg):
    import os
    from conftest import ROOT
    L = pkg.load_library()
    with open(os.path.join(ROOT, "include", "sph_abi.h")) as fh:
        text = fh.read()
    for name in ("sph_aggregate_basis_posgrad_particles", "sph_aggregate_basis_posgrad_query", "sph_aggregate_basis_posgrad_staged", "sph_aggregate_basis_posgrad_host"):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and f"int {name}(" in text, name
    assert "#define SPH_ABI_VERSION 4" in text and "sph_aggregate_basis_posgrad_particles / _query / _staged / _host" in text
