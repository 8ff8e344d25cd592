"""The adjoint of the neighbourhood sums, the extrema with their winners and the routing on the device (sph_aggregate.h) against their
host twins, byte for byte, on the smallest shapes where they can go wrong; the point binning at its edges; the identities with the
forward; sentinels; the proof that a call changes neither the simulation nor a later dispatch; autograd on the device."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import aggregate_adjoint_ref as AJ
from aggregate_ref import radius_of, values_for
import query_scenes as QS
from support import build_example, linked_list_grid, run_example, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
CHANNELS = (1, 5, 16, 33)                  # odd counts, the chunk boundary, several passes
# (weight, self_, delta, moments, radius in h): the MOMENTS contraction with and without DELTA, the reused forward, the three stencils
ADJOINT_CASES = [("one", False, False, True, 1.0), ("poly6", True, True, True, 2.0), ("one", False, True, True, 3.0), ("poly6", True, False, True, 1.0),
                 ("one", False, False, False, 2.0), ("poly6", True, True, False, 1.0)]
QUERY_ADJOINT_CASES = [("one", False, 1.0), ("poly6", True, 2.0), ("one", True, 3.0), ("poly6", False, 3.0)]      # (weight, moments, radius in h)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert got.tobytes() == want.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"


def grads(rows, c, moments, seed=51):
    return np.random.default_rng(seed + c).normal(0.0, 1.0, (rows, 4, c) if moments else (rows, c)).astype(F)


def check_particles(pkg, f, rec, sp, what, channels=CHANNELS, cases=ADJOINT_CASES, fluid_only=False):
    """adjoint, arg and route of particle targets against the host twins."""
    n = len(rec)
    for i, (weight, self_, delta, moments, fac) in enumerate(cases):
        c = channels[i % len(channels)]
        R = radius_of(sp, fac)
        kw = dict(weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments)
        g = grads(n, c, moments)
        same(f.aggregate_adjoint(g, R, **kw), pkg.aggregate_adjoint_host(rec, sp, g, R, **kw), f"adjoint {what} {kw} R {fac} h C {c}")
    for i, (op, self_, delta, fac) in enumerate((("max", False, False, 2.0), ("min", True, True, 1.0), ("max", True, False, 3.0), ("min", False, True, 2.0))):
        c = channels[i % len(channels)]
        R = radius_of(sp, fac)
        kw = dict(op=op, self_=self_, fluid_only=fluid_only, delta=delta)
        x = values_for(n, c)
        x[::9] = x[4]                                                                   # equal values in many rows: the id decides
        out, cnt, arg = f.aggregate_arg(x, R, counts=True, **kw)
        want = pkg.aggregate_arg_host(rec, sp, x, R, counts=True, **kw)
        same(out, want[0], f"arg out {what} {kw}"), same(cnt, want[1], f"arg count {what} {kw}"), same(arg, want[2], f"arg {what} {kw}")
        plain = f.aggregate(x, R, counts=True, **kw)
        same(out, plain[0], "arg out against the plain call"), same(cnt, plain[1], "arg count against the plain call")
        g = grads(n, c, False, seed=61)
        same(f.aggregate_route(arg, g, R, **kw), pkg.aggregate_route_host(rec, sp, arg, g, R, **kw), f"route {what} {kw}")


def check_query(pkg, f, rec, sp, pts, what, channels=CHANNELS, fluid_only=False):
    m = len(pts)
    for i, (weight, moments, fac) in enumerate(QUERY_ADJOINT_CASES):
        c = channels[i % len(channels)]
        R = radius_of(sp, fac)
        kw = dict(weight=weight, fluid_only=fluid_only, moments=moments)
        g = grads(m, c, moments)
        same(f.query_aggregate_adjoint(pts, g, R, **kw), pkg.aggregate_adjoint_host(rec, sp, g, R, points=pts, **kw), f"query adjoint {what} {kw} R {fac} h C {c}")
    for i, (op, fac) in enumerate((("max", 1.0), ("min", 3.0))):
        c = channels[(i + 1) % len(channels)]
        R = radius_of(sp, fac)
        x = values_for(len(rec), c)
        x[::9] = x[4]
        out, cnt, arg = f.query_aggregate_arg(pts, x, R, op=op, fluid_only=fluid_only, counts=True)
        want = pkg.aggregate_arg_host(rec, sp, x, R, points=pts, op=op, fluid_only=fluid_only, counts=True)
        same(out, want[0], f"query arg out {what} {op}"), same(cnt, want[1], f"query arg count {what} {op}"), same(arg, want[2], f"query arg {what} {op}")
        g = grads(m, c, False, seed=62)
        same(f.query_aggregate_route(pts, arg, g, R, op=op, fluid_only=fluid_only),
             pkg.aggregate_route_host(rec, sp, arg, g, R, points=pts, op=op, fluid_only=fluid_only), f"query route {what} {op}")


def test_uniform_every_channel_count(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for shift in range(4):                                                              # every case with every channel count
        check_particles(pkg, f, rec, sp, "uniform", channels=CHANNELS[shift:] + CHANNELS[:shift])
    # SPH_OPT_AGGREGATE_VARIANT steers the reused forward kernel and nothing else: the bytes do not move
    for variant in (1, 8):
        f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, variant)
        check_particles(pkg, f, rec, sp, f"variant {variant}", channels=(16, 5), cases=ADJOINT_CASES[3:])
    f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, 0)
    f.close()


@pytest.mark.parametrize("crowd", [65, 200])
def test_crowded_cell(pkg, crowd):
    rec, sp, start, members = QS.crowded_cell(pkg, crowd)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check_particles(pkg, f, rec, sp, f"crowd {crowd}")
    pts = rec["pos"][::-1, :3].copy()                                                   # as many points in that cell
    check_query(pkg, f, rec, sp, pts, f"crowd {crowd}")
    f.close()


def test_ties_coincident_ghosts_and_non_finite(pkg):
    rec, sp = QS.lattice(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check_particles(pkg, f, rec, sp, "lattice")
    f.close()
    rec, sp, same_ = QS.coincident(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check_particles(pkg, f, rec, sp, "coincident", channels=CHANNELS[1:] + CHANNELS[:1])
    f.close()
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fluid_only in (False, True):
        check_particles(pkg, f, rec, sp, "ghosts", channels=CHANNELS[2:] + CHANNELS[:2], fluid_only=fluid_only)
        check_query(pkg, f, rec, sp, rec["pos"][:333, :3].copy(), "ghosts", fluid_only=fluid_only)
    g = grads(len(rec), 5, True)
    out = f.aggregate_adjoint(g, 1.0, self_=True, fluid_only=True, moments=True)
    assert (out[ghost].view(np.uint32) == 0).all() and out[~ghost].any()                # a ghost's row is +0
    f.close()
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check_particles(pkg, f, rec, sp, "non-finite positions", channels=CHANNELS[3:] + CHANNELS[:3])
    g = grads(len(rec), 5, True)
    out = f.aggregate_adjoint(g, 1.0, moments=True)
    assert (out[[7, 300]].view(np.uint32) == 0).all()
    out = f.aggregate_adjoint(g, 1.0, self_=True, moments=True)
    assert np.array_equal(out[[7, 300]], g[[7, 300], 0])                                # the own slot alone: d = 0, w = 1
    pts = np.random.default_rng(2).permutation(rec["pos"][:, :3])[:500].copy()          # two of them non-finite
    check_query(pkg, f, rec, sp, pts, "non-finite positions")
    f.close()


def test_query_cloud(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for shift in range(4):
        check_query(pkg, f, rec, sp, pts, "query cloud", channels=CHANNELS[shift:] + CHANNELS[:shift])
    # a torch device tensor of (m, 4) points and of g is used in place
    p4 = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, np.ones((len(pts), 1), F)], axis=1))).cuda()
    g = grads(len(pts), 5, True)
    gt = torch.from_numpy(g).cuda()
    out = f.query_aggregate_adjoint(p4, gt, 1.0, weight="poly6", moments=True, device=True)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(rec), 5)
    same(out.cpu().numpy(), pkg.aggregate_adjoint_host(rec, sp, g, 1.0, points=pts, weight="poly6", moments=True), "device tensors in place")
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), g.view(np.uint32)) and np.array_equal(p4.cpu().numpy()[:, :3].view(np.uint32), pts.view(np.uint32))
    f.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 701])
def test_point_binning_counts(pkg, m):
    rec, sp, pts = QS.query_cloud(pkg)
    pts = pts[:m]
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for c, moments, fac in ((5, True, 2.0), (16, False, 3.0)):
        g = grads(m, c, moments)
        R = radius_of(sp, fac)
        want = pkg.aggregate_adjoint_host(rec, sp, g, R, points=pts, weight="poly6", moments=moments)
        assert want.any()
        same(f.query_aggregate_adjoint(pts, g, R, weight="poly6", moments=moments), want, f"m {m} C {c}")
        same(f.query_aggregate_adjoint(pts, g, R, weight="poly6", moments=moments), want, f"m {m} C {c}, again")
    f.close()


def test_point_binning_edges(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    lo, dims, cs = QS.grid(pkg, sp)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rng = np.random.default_rng(6)
    one_cell = (lo + (np.array([3, 2, 4], F) + F(0.05) + F(0.9) * rng.random((300, 3)).astype(F)) * cs).astype(F)       # all 300 points in one cell
    g = grads(300, 5, True)
    for R in (radius_of(sp, 1.0), radius_of(sp, 3.0)):
        want = pkg.aggregate_adjoint_host(rec, sp, g, R, points=one_cell, moments=True)
        assert want.any()
        same(f.query_aggregate_adjoint(one_cell, g, R, moments=True), want, "300 points in one cell")
        # reversed points change out only as the host twin says (the order inside the cell is the point index)
        rev = pkg.aggregate_adjoint_host(rec, sp, g[::-1].copy(), R, points=one_cell[::-1].copy(), moments=True)
        same(f.query_aggregate_adjoint(one_cell[::-1].copy(), g[::-1].copy(), R, moments=True), rev, "reversed points")
        assert rev.tobytes() != want.tobytes() and np.allclose(rev, want, rtol=0, atol=1e-3)
    bad = np.full((70, 3), np.nan, F)
    bad[1::2] = np.inf
    out = f.query_aggregate_adjoint(bad, grads(70, 3, False), 1.0)
    assert out.shape == (1000, 3) and (out.view(np.uint32) == 0).all()                   # all points non-finite: +0 everywhere
    out = f.query_aggregate_adjoint(np.zeros((0, 3), F), np.zeros((0, 4, 2), F), 1.0, moments=True)
    assert out.shape == (1000, 2) and (out.view(np.uint32) == 0).all()                   # m = 0: out is zeroed
    arg = np.full((70, 3), -1, np.int32)
    assert (f.query_aggregate_route(bad, arg, grads(70, 3, False), 1.0).view(np.uint32) == 0).all()
    f.close()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    f = pkg.SPHFluidGPU.from_particles(none, sp)
    assert f.query_aggregate_adjoint(one_cell, g, 1.0, moments=True).shape == (0, 5) and f.aggregate_adjoint(np.zeros((0, 3), F), 1.0).shape == (0, 3)
    out, arg = f.query_aggregate_arg(one_cell, np.zeros((0, 2), F), 1.0)
    assert out.shape == (300, 2) and (arg == -1).all()
    f.close()


def test_identities_and_repeatability(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for weight in ("one", "poly6"):
        for self_ in (False, True):
            for delta in (False, True):
                for fluid_only in (False, True):
                    g = grads(len(rec), 5, False)
                    kw = dict(weight=weight, self_=self_, fluid_only=fluid_only, delta=delta)
                    a = f.aggregate_adjoint(g, 1.0, **kw)
                    same(a, f.aggregate(g, 1.0, **kw), f"adjoint = forward {kw}")
                    same(a, pkg.aggregate_adjoint_host(rec, sp, g, 1.0, **kw), f"adjoint = host twin {kw}")
    g = grads(len(rec), 16, True)
    a = f.aggregate_adjoint(g, 1.0, weight="poly6", delta=True, moments=True)
    same(f.aggregate_adjoint(g, 1.0, weight="poly6", delta=True, moments=True), a, "two calls in a row")
    # the dot-product identity on the device, within the bound of aggregate_adjoint_ref
    x = values_for(len(rec), 16, seed=41)
    y = f.aggregate(x, 1.0, weight="poly6", delta=True, moments=True)
    T, kmax = AJ.magnitudes(pkg, rec, sp, x, g, 1.0, weight="poly6", delta=True, moments=True)
    lhs, rhs = float((y.astype(np.float64) * g).sum()), float((x.astype(np.float64) * a).sum())
    print(f"<Ax, g> {lhs:.9g}, <x, A^T g> {rhs:.9g}, |difference| / bound {abs(lhs - rhs) / AJ.dot_bound(T, kmax):.3g}")
    assert abs(lhs - rhs) <= AJ.dot_bound(T, kmax)
    f.close()


def test_sentinels(pkg):
    """Every row of out and nothing beyond n * C is written; g, arg and the points never."""
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    L = pkg.load_library()
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    pt = torch.from_numpy(p4).cuda()
    MOM, MAX = pkg.SPH_AGGREGATE_MOMENTS, pkg.SPH_AGGREGATE_MAX
    for c in (5, 16):
        words = n * c
        gp, gq = torch.from_numpy(grads(n, c, True)).cuda(), torch.from_numpy(grads(m, c, True)).cuda()
        argp = torch.from_numpy(np.random.default_rng(1).integers(-1, n, (n, c)).astype(np.int32)).cuda()
        argq = torch.from_numpy(np.random.default_rng(2).integers(-1, n, (m, c)).astype(np.int32)).cuda()
        held = [t.clone() for t in (gp, gq, argp, argq, pt)]
        info = pkg.SphAggregateInfo()
        calls = {
            "adjoint, particles": lambda o: L.sph_aggregate_adjoint_particles(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=c, flags=MOM)), vp(gp.data_ptr()), o, C.byref(info)),
            "adjoint, reused forward": lambda o: L.sph_aggregate_adjoint_particles(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=c)), vp(gp.data_ptr()), o, C.byref(info)),
            "adjoint, query": lambda o: L.sph_aggregate_adjoint_query(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=c, flags=MOM)), vp(pt.data_ptr()), m, vp(gq.data_ptr()), o, C.byref(info)),
            "route, particles": lambda o: L.sph_aggregate_route_particles(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=c, op=MAX)), vp(argp.data_ptr()), vp(gp.data_ptr()), o, C.byref(info)),
            "route, query": lambda o: L.sph_aggregate_route_query(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=c, op=MAX)), vp(pt.data_ptr()), m, vp(argq.data_ptr()), vp(gq.data_ptr()), o, C.byref(info)),
        }
        for name, call in calls.items():
            buf = torch.full((words + 64,), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert call(vp(buf.data_ptr() + 128)) == 0, name
            f.sync()
            got = buf.cpu().numpy()
            assert np.isnan(got[:32]).all() and np.isnan(got[32 + words:]).all() and not np.isnan(got[32:32 + words]).any(), name
            assert (info.rows, info.channels, info.stencil) == (n, c, 2) and info.planes == (4 if "adjoint, particles" == name or "adjoint, query" == name else 1), name
        for t, h in zip((gp, gq, argp, argq, pt), held):
            assert torch.equal(t.view(torch.int32), h.view(torch.int32))
    # the arg call: out, count and arg inside their sentinels
    x = torch.from_numpy(values_for(n, 5)).cuda()
    out = torch.full((m * 5 + 64,), 12345.0, dtype=torch.float32, device="cuda")
    arg = torch.full((m * 5 + 64,), 77, dtype=torch.int32, device="cuda")
    cnt = torch.full((m + 64,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    assert L.sph_aggregate_arg_query(f._h, C.byref(pkg.aggregate_config(radius=1.0, channels=5, op=MAX)), vp(pt.data_ptr()), m, vp(x.data_ptr()),
                                     vp(out.data_ptr() + 128), vp(cnt.data_ptr() + 128), vp(arg.data_ptr() + 128), C.byref(info)) == 0
    f.sync()
    o, a, k = out.cpu().numpy(), arg.cpu().numpy(), cnt.cpu().numpy()
    assert (o[:32] == 12345.0).all() and (o[32 + m * 5:] == 12345.0).all() and (a[:32] == 77).all() and (a[32 + m * 5:] == 77).all()
    assert (k[:32] == 77).all() and (k[32 + m:] == 77).all()
    want = pkg.aggregate_arg_host(rec, sp, values_for(n, 5), 1.0, points=pts, counts=True)
    same(o[32:32 + m * 5].reshape(m, 5), want[0], "arg out"), same(a[32:32 + m * 5].reshape(m, 5), want[2], "arg"), same(k[32:32 + m].view(np.uint32), want[1], "count")
    f.close()


def test_refusals(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n, h = len(rec), sp.param_h
    g = torch.zeros((n, 4, 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    arg = torch.full((n, 4), 3, dtype=torch.int32, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    good = dict(radius=h, channels=4)
    SUM, MAX = pkg.SPH_AGGREGATE_SUM, pkg.SPH_AGGREGATE_MAX
    p = lambda t: None if t is None else vp(t.data_ptr())

    def adjoint(e, cfg, g_=g, out_=out):
        return L.sph_aggregate_adjoint_particles(e, C.byref(cfg), p(g_), p(out_), C.byref(info))

    def adjoint_query(e, cfg, m=4, out_=out, pts_=pts):
        return L.sph_aggregate_adjoint_query(e, C.byref(cfg), p(pts_), m, p(g), p(out_), C.byref(info))

    def route(e, cfg, arg_=arg):
        return L.sph_aggregate_route_particles(e, C.byref(cfg), p(arg_), p(g), p(out), C.byref(info))

    def winners(e, cfg, arg_=arg):
        return L.sph_aggregate_arg_particles(e, C.byref(cfg), p(g), p(out), None, p(arg_), C.byref(info))

    with slab_engine(pkg, rec, sp) as slab:
        assert adjoint(slab._h, pkg.aggregate_config(**good)) == -3 and b"slab" in L.sph_last_error()
        assert adjoint_query(slab._h, pkg.aggregate_config(**good)) == -3 and route(slab._h, pkg.aggregate_config(op=MAX, **good)) == -3
        assert winners(slab._h, pkg.aggregate_config(op=MAX, **good)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        assert adjoint(f._h, pkg.aggregate_config(**good)) == -3 and adjoint_query(f._h, pkg.aggregate_config(**good)) == -3
        assert route(f._h, pkg.aggregate_config(op=MAX, **good)) == -3 and winners(f._h, pkg.aggregate_config(op=MAX, **good)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.aggregate_adjoint(g[:, 0].contiguous())
    assert adjoint(None, pkg.aggregate_config(**good)) == -1 and adjoint(f._h, pkg.aggregate_config(**good), g_=None) == -1
    assert adjoint(f._h, pkg.aggregate_config(**good), out_=None) == -1
    for op in (pkg.SPH_AGGREGATE_MEAN, MAX, pkg.SPH_AGGREGATE_MIN, 4):
        assert adjoint(f._h, pkg.aggregate_config(op=op, **good)) == -1 and adjoint_query(f._h, pkg.aggregate_config(op=op, **good)) == -1
    for bad in (dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129), dict(radius=0.0), dict(radius=3.01 * h)):
        assert adjoint(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
        assert adjoint_query(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):
        assert adjoint_query(f._h, pkg.aggregate_config(flags=flag, **good)) == -1
    assert adjoint_query(f._h, pkg.aggregate_config(**good), m=1 << 31) == -1
    flat = g.view(-1)
    assert adjoint(f._h, pkg.aggregate_config(**good), g_=flat, out_=flat[n * 4 - 4:]) == -1 and b"overlap" in L.sph_last_error()
    assert adjoint_query(f._h, pkg.aggregate_config(**good), out_=flat[8:], pts_=flat) == -1
    assert route(f._h, pkg.aggregate_config(op=SUM, **good)) == -1 and route(f._h, pkg.aggregate_config(op=MAX, **good), arg_=None) == -1
    assert winners(f._h, pkg.aggregate_config(op=SUM, **good)) == -1 and winners(f._h, pkg.aggregate_config(op=MAX, **good), arg_=None) == -1
    f.sync()
    assert (out == 7.0).all().item() and (arg == 3).all().item() and (g == 0).all().item()      # no refused call wrote anything
    assert adjoint(f._h, pkg.aggregate_config(**good)) == 0                                     # ... and the valid call works afterwards
    f.sync()
    assert (out == 0.0).all().item()
    f.close()


def test_adjoint_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()
    g = grads(len(rec), 5, True)
    gq = grads(len(pts), 5, False)
    arg = np.random.default_rng(3).integers(-1, len(rec), (len(pts), 5)).astype(np.int32)

    def probe(f):
        f.aggregate_adjoint(g, 2.0 * sp.param_h, weight="poly6", self_=True, delta=True, moments=True)
        f.aggregate_adjoint(g[:, 0].copy(), delta=True)
        f.query_aggregate_adjoint(pts, gq, sp.param_h)
        f.query_aggregate_route(pts, arg, gq, sp.param_h)
        f.aggregate_arg(g[:, 1].copy(), op="min")

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


AUTOGRAD_CASES = [dict(op="sum"), dict(op="sum", weight="poly6", self_=True, delta=True, moments=True), dict(op="mean", delta=True),
                  dict(op="mean", weight="poly6", self_=True), dict(op="max", self_=True), dict(op="min", delta=True)]


def test_autograd_on_the_device(pkg):
    import torch
    rec, sp = QS.uniform(pkg, 1000, 21)
    n = len(rec)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    host = pkg.HostAggregateBackend(rec, sp)
    x = values_for(n, 5)
    x[::9] = x[4]
    for kw in AUTOGRAD_CASES:
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        y = f.aggregate_autograd(xt, 1.0, **kw)
        same(y.detach().cpu().numpy(), f.aggregate(x, 1.0, **kw), f"forward {kw}")
        g = np.random.default_rng(8).normal(0.0, 1.0, tuple(y.shape)).astype(F)
        (y * torch.from_numpy(g).cuda()).sum().backward()
        xh = torch.from_numpy(x).requires_grad_(True)
        (pkg.aggregate_autograd(host, None, xh, 1.0, **kw) * torch.from_numpy(g)).sum().backward()
        same(xt.grad.cpu().numpy(), xh.grad.numpy(), f"values.grad {kw}")
    rec2, sp2, pts = QS.query_cloud(pkg)
    f2 = pkg.SPHFluidGPU.from_particles(rec2, sp2)
    host2 = pkg.HostAggregateBackend(rec2, sp2)
    x2 = values_for(len(rec2), 3)
    for kw in (dict(op="sum", weight="poly6", moments=True), dict(op="mean"), dict(op="mean", weight="poly6"), dict(op="min")):
        xt = torch.from_numpy(x2).cuda().requires_grad_(True)
        y = f2.query_aggregate_autograd(pts, xt, 1.0, **kw)
        same(y.detach().cpu().numpy(), f2.query_aggregate(pts, x2, 1.0, **kw), f"query forward {kw}")
        g = np.random.default_rng(9).normal(0.0, 1.0, tuple(y.shape)).astype(F)
        (y * torch.from_numpy(g).cuda()).sum().backward()
        xh = torch.from_numpy(x2).requires_grad_(True)
        p4 = np.zeros((len(pts), 4), F)
        p4[:, :3] = pts
        (pkg.aggregate_autograd(host2, p4, xh, 1.0, **kw) * torch.from_numpy(g)).sum().backward()
        same(xt.grad.cpu().numpy(), xh.grad.numpy(), f"query values.grad {kw}")
    f2.close()
    # a dispatch between forward and backward
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = f.aggregate_autograd(xt, 1.0)
    f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = f.aggregate_autograd(xt, 1.0, check_state=False)
    f.DispatchCompute()
    y.sum().backward()
    assert xt.grad is not None and tuple(xt.grad.shape) == (n, 5)
    f.close()


def test_scatter_to_particles_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "scatter_to_particles", tmp_path, werror=True), ["20000"], timeout=120)
    assert res.returncode == 0 and "scatter_to_particles OK" in res.stdout
