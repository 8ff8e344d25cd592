"""Position gradients of the neighbourhood sums on the device (sph_posgrad.h) against the host twin, byte for byte, on the smallest
shapes where the kernels can go wrong (the scenes of test_gpu_aggregate_adjoint); sentinels; the proof that a call changes neither the
simulation nor a later dispatch; the refusals; autograd on the device; the example."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import aggregate_posgrad_ref as PR
from aggregate_ref import radius_of, values_for
import query_scenes as QS
from support import build_example, linked_list_grid, run_example, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
CHANNELS = (1, 5, 16, 33)                  # a lone lane, a group tail, an exact fit, a partial last pass of the butterfly's widest group
# (weight, self_, delta, moments, radius in h): every flag combination with a walk, the three stencils
PARTICLE_CASES = [("poly6", False, False, False, 1.0), ("poly6", True, True, True, 2.0), ("one", False, True, True, 3.0), ("poly6", True, False, True, 1.0),
                  ("poly6", False, True, False, 2.0), ("one", True, False, True, 1.0)]
QUERY_CASES = [("poly6", False, 1.0), ("poly6", True, 2.0), ("one", True, 3.0), ("poly6", False, 3.0)]      # (weight, moments, radius in h)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert got.tobytes() == want.tobytes(), f"{what}: {len(bad)} rows differ, first {bad[:5]}"


def grads(rows, c, moments, seed=51):
    return np.random.default_rng(seed + c).normal(0.0, 1.0, (rows, 4, c) if moments else (rows, c)).astype(F)


def check_particles(pkg, f, rec, sp, what, channels=CHANNELS, cases=PARTICLE_CASES, fluid_only=False):
    n = len(rec)
    for i, (weight, self_, delta, moments, fac) in enumerate(cases):
        c = channels[i % len(channels)]
        R = radius_of(sp, fac)
        kw = dict(weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments)
        x, g = values_for(n, c, seed=43), grads(n, c, moments)
        want = pkg.aggregate_position_grad_host(rec, sp, x, g, R, **kw)
        assert want.any()
        same(f.aggregate_position_grad(x, g, R, **kw), want, f"particles {what} {kw} R {fac} h C {c}")


def check_query(pkg, f, rec, sp, pts, what, channels=CHANNELS, fluid_only=False):
    m = len(pts)
    for i, (weight, moments, fac) in enumerate(QUERY_CASES):
        c = channels[i % len(channels)]
        R = radius_of(sp, fac)
        kw = dict(weight=weight, fluid_only=fluid_only, moments=moments)
        x, g = values_for(len(rec), c, seed=44), grads(m, c, moments)
        wp, wx = pkg.aggregate_position_grad_host(rec, sp, x, g, R, points=pts, **kw)
        gp, gx = f.query_aggregate_position_grad(pts, x, g, R, **kw)
        same(gp, wp, f"query points {what} {kw} R {fac} h C {c}")
        same(gx, wx, f"query particles {what} {kw} R {fac} h C {c}")


def test_uniform_every_channel_count(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for shift in range(4):                                                              # every case with every channel count
        check_particles(pkg, f, rec, sp, "uniform", channels=CHANNELS[shift:] + CHANNELS[:shift])
    # the most registers and the widest group: two channels per lane of a whole wave
    check_particles(pkg, f, rec, sp, "uniform", channels=(128,), cases=[("poly6", True, True, True, 2.0)])
    # weight ONE without MOMENTS: +0 everywhere, also with SELF and DELTA
    out = f.aggregate_position_grad(values_for(1000, 5), grads(1000, 5, False), 1.0, weight="one", self_=True, delta=True)
    assert out.shape == (1000, 3) and (out.view(np.uint32) == 0).all()
    # SELF does not move a byte
    x, g = values_for(1000, 5), grads(1000, 5, True)
    same(f.aggregate_position_grad(x, g, 1.0, weight="poly6", moments=True, self_=True), f.aggregate_position_grad(x, g, 1.0, weight="poly6", moments=True), "SELF")
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
    check_query(pkg, f, rec, sp, rec["pos"][::2, :3].copy(), "coincident")              # points on the particles: d = 0 pairs
    f.close()
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fluid_only in (False, True):
        check_particles(pkg, f, rec, sp, "ghosts", channels=CHANNELS[2:] + CHANNELS[:2], fluid_only=fluid_only)
        check_query(pkg, f, rec, sp, rec["pos"][:333, :3].copy(), "ghosts", fluid_only=fluid_only)
    out = f.aggregate_position_grad(values_for(len(rec), 5), grads(len(rec), 5, True), 1.0, weight="poly6", fluid_only=True, moments=True)
    assert (out[ghost].view(np.uint32) == 0).all() and out[~ghost].any()                # a ghost's row is +0
    gx = f.query_aggregate_position_grad(rec["pos"][:333, :3].copy(), values_for(len(rec), 5), grads(333, 5, True), 1.0, weight="poly6", fluid_only=True, moments=True)[1]
    assert (gx[ghost].view(np.uint32) == 0).all() and gx[~ghost].any()
    f.close()
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check_particles(pkg, f, rec, sp, "non-finite positions", channels=CHANNELS[3:] + CHANNELS[:3])
    out = f.aggregate_position_grad(values_for(1000, 5), grads(1000, 5, True), 1.0, weight="poly6", moments=True, delta=True)
    assert (out[[7, 300]].view(np.uint32) == 0).all() and np.isfinite(out).all()
    pts = np.random.default_rng(2).permutation(rec["pos"][:, :3])[:500].copy()          # two of them non-finite
    check_query(pkg, f, rec, sp, pts, "non-finite positions")
    bad = np.flatnonzero(~np.isfinite(pts).all(axis=1))
    gp = f.query_aggregate_position_grad(pts, values_for(1000, 5), grads(500, 5, True), 1.0, weight="poly6", moments=True)[0]
    assert len(bad) == 2 and (gp[bad].view(np.uint32) == 0).all()
    f.close()


def test_query_cloud_clamped_cells_and_null_outputs(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)                                                  # points and particles beyond the grid's faces
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for shift in range(4):
        check_query(pkg, f, rec, sp, pts, "query cloud", channels=CHANNELS[shift:] + CHANNELS[:shift])
    check_query(pkg, f, rec, sp, pts, "query cloud", channels=(128,))
    lo, dims, cs = QS.grid(pkg, sp)
    far = ((pts < lo) | (pts > lo + dims.astype(F) * cs)).any(axis=1)
    x, g = values_for(n, 5), grads(m, 5, True)
    wp, wx = pkg.aggregate_position_grad_host(rec, sp, x, g, 1.0, points=pts, weight="poly6", moments=True)
    assert wp[far].any()                                                                # points in clamped cells take part
    # one null output at a time: the other's bytes
    gp, none = f.query_aggregate_position_grad(pts, x, g, 1.0, weight="poly6", moments=True, want_particles=False)
    assert none is None
    same(gp, wp, "points alone")
    none, gx = f.query_aggregate_position_grad(pts, x, g, 1.0, weight="poly6", moments=True, want_points=False)
    assert none is None
    same(gx, wx, "particles alone")
    # device tensors are used in place and never written
    p4 = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, np.ones((m, 1), F)], axis=1))).cuda()
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    dp, dx = f.query_aggregate_position_grad(p4, xt, gt, 1.0, weight="poly6", moments=True, device=True)
    assert dp.is_cuda and tuple(dp.shape) == (m, 3) and tuple(dx.shape) == (n, 3)
    same(dp.cpu().numpy(), wp, "device tensors: points"), same(dx.cpu().numpy(), wx, "device tensors: particles")
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), g.view(np.uint32)) and np.array_equal(xt.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # m = 0: the particles' output is zeroed; all points non-finite: +0 everywhere
    gp, gx = f.query_aggregate_position_grad(np.zeros((0, 3), F), x, np.zeros((0, 4, 5), F), 1.0, weight="poly6", moments=True)
    assert gp.shape == (0, 3) and gx.shape == (n, 3) and (gx.view(np.uint32) == 0).all()
    bad = np.full((70, 3), np.nan, F)
    gp, gx = f.query_aggregate_position_grad(bad, x, grads(70, 5, False), 1.0, weight="poly6")
    assert (gp.view(np.uint32) == 0).all() and (gx.view(np.uint32) == 0).all()
    # two calls in a row: the same bytes
    same(f.query_aggregate_position_grad(pts, x, g, 1.0, weight="poly6", moments=True)[1], wx, "again")
    f.close()
    empty = pkg.SPHFluidGPU.from_particles(np.zeros(0, pkg.PARTICLE_DTYPE), sp)         # n = 0: success, nothing to write
    assert empty.aggregate_position_grad(np.zeros((0, 2), F), np.zeros((0, 2), F), 1.0, weight="poly6").shape == (0, 3)
    empty.close()


def test_sentinels_and_the_staged_call(pkg):
    """Every row of the outputs and nothing beyond them is written; values, g and the points never."""
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    L = pkg.load_library()
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    pt = torch.from_numpy(p4).cuda()
    POLY6 = pkg.SPH_AGGREGATE_WEIGHT_POLY6
    info = pkg.SphAggregateInfo()
    for c, flags in ((5, pkg.SPH_AGGREGATE_MOMENTS), (16, 0), (128, pkg.SPH_AGGREGATE_MOMENTS)):
        planes = 4 if flags else 1
        x = torch.from_numpy(values_for(n, c)).cuda()
        gp, gq = torch.from_numpy(grads(n, c, bool(flags))).cuda(), torch.from_numpy(grads(m, c, bool(flags))).cuda()
        held = [t.clone() for t in (x, gp, gq, pt)]
        cfg = pkg.aggregate_config(radius=1.0, channels=c, weight=POLY6, flags=flags)
        a = torch.full((n * 3 + 64,), float("nan"), dtype=torch.float32, device="cuda")
        b = torch.full((m * 3 + 64,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert L.sph_aggregate_posgrad_particles(f._h, C.byref(cfg), vp(x.data_ptr()), vp(gp.data_ptr()), vp(a.data_ptr() + 128), C.byref(info)) == 0
        f.sync()
        got = a.cpu().numpy()
        assert np.isnan(got[:32]).all() and np.isnan(got[32 + n * 3:]).all() and not np.isnan(got[32:32 + n * 3]).any()
        assert (info.rows, info.channels, info.planes, info.stencil) == (n, c, planes, 2)
        a.fill_(float("nan"))
        torch.cuda.synchronize()
        assert L.sph_aggregate_posgrad_query(f._h, C.byref(cfg), vp(pt.data_ptr()), m, vp(x.data_ptr()), vp(gq.data_ptr()), vp(b.data_ptr() + 128), vp(a.data_ptr() + 128),
                                             C.byref(info)) == 0
        f.sync()
        for t, k in ((a, n), (b, m)):
            got = t.cpu().numpy()
            assert np.isnan(got[:32]).all() and np.isnan(got[32 + k * 3:]).all() and not np.isnan(got[32:32 + k * 3]).any()
        assert (info.rows, info.channels, info.planes) == (m, c, planes)
        for t, h in zip((x, gp, gq, pt), held):
            assert torch.equal(t.view(torch.int32), h.view(torch.int32))
    # the staged call round-trips host arrays: the twin's bytes
    x, g, gq = values_for(n, 5), grads(n, 5, True), grads(m, 5, True)
    cfg = pkg.aggregate_config(radius=1.0, channels=5, weight=POLY6, flags=pkg.SPH_AGGREGATE_MOMENTS | pkg.SPH_AGGREGATE_DELTA)
    p = lambda arr: arr.ctypes.data_as(vp)
    out = np.full((n, 3), 7.0, F)
    assert L.sph_aggregate_posgrad_staged(f._h, C.byref(cfg), None, 0, p(x), p(g), None, p(out), C.byref(info)) == 0
    same(out, pkg.aggregate_position_grad_host(rec, sp, x, g, 1.0, weight="poly6", delta=True, moments=True), "staged, particles")
    cfg = pkg.aggregate_config(radius=1.0, channels=5, weight=POLY6, flags=pkg.SPH_AGGREGATE_MOMENTS)
    op, ox = np.full((m, 3), 7.0, F), np.full((n, 3), 7.0, F)
    assert L.sph_aggregate_posgrad_staged(f._h, C.byref(cfg), p(p4), m, p(x), p(gq), p(op), p(ox), C.byref(info)) == 0
    wp, wx = pkg.aggregate_position_grad_host(rec, sp, x, gq, 1.0, points=pts, weight="poly6", moments=True)
    same(op, wp, "staged, points"), same(ox, wx, "staged, query particles")
    f.close()


def test_refusals(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n, h = len(rec), sp.param_h
    x = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    g = torch.zeros((n, 4, 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    outp = torch.full((4, 3), 7.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    good = dict(radius=h, channels=4, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6)
    p = lambda t: None if t is None else vp(t.data_ptr())

    def particles(e, cfg, x_=x, g_=g, out_=out):
        return L.sph_aggregate_posgrad_particles(e, C.byref(cfg), p(x_), p(g_), p(out_), C.byref(info))

    def query(e, cfg, m=4, pts_=pts, outp_=outp, out_=out):
        return L.sph_aggregate_posgrad_query(e, C.byref(cfg), p(pts_), m, p(x), p(g), p(outp_), p(out_), C.byref(info))

    with slab_engine(pkg, rec, sp) as slab:
        assert particles(slab._h, pkg.aggregate_config(**good)) == -3 and b"slab" in L.sph_last_error()
        assert query(slab._h, pkg.aggregate_config(**good)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        assert particles(f._h, pkg.aggregate_config(**good)) == -3 and query(f._h, pkg.aggregate_config(**good)) == -3
        assert particles(f._h, pkg.aggregate_config(radius=h, channels=4)) == -3         # also where no walk would be launched
        with pytest.raises(pkg.SphError, match="-3"):
            f.aggregate_position_grad(x, g[:, 0].contiguous(), weight="poly6")
    assert particles(None, pkg.aggregate_config(**good)) == -1 and particles(f._h, pkg.aggregate_config(**good), x_=None) == -1
    assert particles(f._h, pkg.aggregate_config(**good), g_=None) == -1 and particles(f._h, pkg.aggregate_config(**good), out_=None) == -1
    assert query(f._h, pkg.aggregate_config(**good), outp_=None, out_=None) == -1       # both outputs null
    assert query(f._h, pkg.aggregate_config(**good), pts_=None) == -1
    for op in (pkg.SPH_AGGREGATE_MEAN, pkg.SPH_AGGREGATE_MAX, pkg.SPH_AGGREGATE_MIN, 4):
        assert particles(f._h, pkg.aggregate_config(op=op, **good)) == -1 and query(f._h, pkg.aggregate_config(op=op, **good)) == -1
    for bad in (dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129), dict(radius=0.0), dict(radius=3.01 * h)):
        assert particles(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
        assert query(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):
        assert query(f._h, pkg.aggregate_config(flags=flag, **good)) == -1
    assert query(f._h, pkg.aggregate_config(**good), m=1 << 31) == -1
    flat = g.view(-1)
    assert particles(f._h, pkg.aggregate_config(**good), g_=flat, out_=flat[n * 4 - 4:]) == -1 and b"overlap" in L.sph_last_error()
    assert particles(f._h, pkg.aggregate_config(**good), x_=flat, out_=flat[8:]) == -1
    assert query(f._h, pkg.aggregate_config(**good), outp_=flat[4:], out_=flat) == -1   # the outputs overlap each other
    assert query(f._h, pkg.aggregate_config(**good), pts_=flat, outp_=flat[8:]) == -1
    f.sync()
    assert (out == 7.0).all().item() and (outp == 7.0).all().item() and (g == 0).all().item()   # no refused call wrote anything
    assert particles(f._h, pkg.aggregate_config(**good)) == 0                                   # ... and the valid call works afterwards
    f.sync()
    assert (out == 0.0).all().item()
    f.close()


def test_a_call_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()
    x, g, gq = values_for(len(rec), 5), grads(len(rec), 5, True), grads(len(pts), 5, False)

    def probe(f):
        f.aggregate_position_grad(x, g, 2.0 * sp.param_h, weight="poly6", self_=True, delta=True, moments=True)
        f.aggregate_position_grad(x, g[:, 0].copy(), weight="poly6")
        f.query_aggregate_position_grad(pts, x, gq, sp.param_h, weight="poly6")
        f.positions(device=True)

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def test_autograd_on_the_device(pkg):
    import torch
    rec, sp = QS.uniform(pkg, 1000, 21)
    n = len(rec)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    host = pkg.HostAggregateBackend(rec, sp)
    x = values_for(n, 5)
    pos = f.positions(device=True)
    assert pos.is_cuda and tuple(pos.shape) == (n, 3)
    same(pos.cpu().numpy(), np.ascontiguousarray(rec["pos"][:, :3]), "positions(device=True)")
    same(f.positions(), np.ascontiguousarray(rec["pos"][:, :3]), "positions()")
    # sum: positions.grad is the direct call, byte for byte; the forward has the bytes of aggregate(device=True)
    for kw in (dict(weight="poly6"), dict(weight="poly6", self_=True, delta=True, moments=True), dict(weight="one", moments=True)):
        xt, pt = torch.from_numpy(x).cuda().requires_grad_(True), pos.clone().requires_grad_(True)
        y = f.aggregate_autograd(xt, 1.0, positions=pt, **kw)
        same(y.detach().cpu().numpy(), f.aggregate(x, 1.0, **kw), f"forward {kw}")
        g = np.random.default_rng(8).normal(0.0, 1.0, tuple(y.shape)).astype(F)
        (y * torch.from_numpy(g).cuda()).sum().backward()
        same(pt.grad.cpu().numpy(), f.aggregate_position_grad(x, g, 1.0, **kw), f"positions.grad {kw}")
        same(xt.grad.cpu().numpy(), f.aggregate_adjoint(g, 1.0, **kw), f"values.grad {kw}")
    # mean: within the CPU test's bound (aggregate_posgrad_ref.mean_bound) of the host backend; torch's elementwise kernels sit between the calls
    for kw in (dict(op="mean", weight="poly6", self_=True), dict(op="mean", weight="poly6", delta=True), dict(op="max")):
        xt, pt = torch.from_numpy(x).cuda().requires_grad_(True), pos.clone().requires_grad_(True)
        y = f.aggregate_autograd(xt, 1.0, positions=pt, **kw)
        g = np.random.default_rng(9).normal(0.0, 1.0, tuple(y.shape)).astype(F)
        (y * torch.from_numpy(g).cuda()).sum().backward()
        xh, ph = torch.from_numpy(x).requires_grad_(True), host.positions().requires_grad_(True)
        yh = pkg.aggregate_autograd(host, None, xh, 1.0, positions=ph, **kw)
        (yh * torch.from_numpy(g)).sum().backward()
        got, want = pt.grad.cpu().numpy(), ph.grad.numpy()
        if kw["op"] == "max":
            assert (got.view(np.uint32) == 0).all() and (want.view(np.uint32) == 0).all()
            continue
        dense = pkg.aggregate_host(rec, sp, x, 1.0, **kw).astype(np.float64)           # (the fp32 mean stands in for the dense float64 one here)
        bound = PR.mean_bound(pkg, rec, sp, x, g, dense, 1.0, weight="poly6", self_=kw.get("self_", False), delta=kw.get("delta", False))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"{kw}: largest |gradient| {np.abs(want).max():.4g}, largest device - host {err.max():.3g}, largest over bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert np.abs(want).max() > 0 and (err <= bound).all()
    # a positions tensor that is not the engine's raises; a dispatch between forward and backward raises
    moved = pos.clone()
    moved[17, 1] += 1e-3
    with pytest.raises(pkg.SphError, match="positions"):
        f.aggregate_autograd(torch.from_numpy(x).cuda(), 1.0, weight="poly6", positions=moved.requires_grad_(True))
    # query targets: points.grad and positions.grad are the direct call's two outputs
    rec2, sp2, pts = QS.query_cloud(pkg)
    f2 = pkg.SPHFluidGPU.from_particles(rec2, sp2)
    x2 = values_for(len(rec2), 3)
    for width in (3, 4):
        kw = dict(weight="poly6", moments=True)
        xt, pt = torch.from_numpy(x2).cuda().requires_grad_(True), f2.positions(device=True).requires_grad_(True)
        full = pts if width == 3 else np.concatenate([pts, np.ones((len(pts), 1), F)], axis=1)
        qt = torch.from_numpy(np.ascontiguousarray(full)).cuda().requires_grad_(True)
        y = f2.query_aggregate_autograd(qt, xt, 1.0, positions=pt, points_grad=True, **kw)
        same(y.detach().cpu().numpy(), f2.query_aggregate(pts, x2, 1.0, **kw), "query forward")
        g = np.random.default_rng(10).normal(0.0, 1.0, tuple(y.shape)).astype(F)
        (y * torch.from_numpy(g).cuda()).sum().backward()
        wp, wx = f2.query_aggregate_position_grad(pts, x2, g, 1.0, **kw)
        same(qt.grad.cpu().numpy()[:, :3].copy(), wp, f"points.grad, width {width}")
        same(pt.grad.cpu().numpy(), wx, "positions.grad")
        assert tuple(qt.grad.shape) == (len(pts), width) and not qt.grad[:, 3:].any().item()
    # without the keywords a points tensor that requires grad gets None
    qt = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, np.ones((len(pts), 1), F)], axis=1))).cuda().requires_grad_(True)
    xt = torch.from_numpy(x2).cuda().requires_grad_(True)
    f2.query_aggregate_autograd(qt, xt, 1.0, weight="poly6").sum().backward()
    assert qt.grad is None and xt.grad is not None
    f2.close()
    xt, pt = torch.from_numpy(x).cuda().requires_grad_(True), pos.clone().requires_grad_(True)
    y = f.aggregate_autograd(xt, 1.0, weight="poly6", positions=pt)
    f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    f.close()


def test_position_gradient_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "position_gradient", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "position_gradient OK" in res.stdout
