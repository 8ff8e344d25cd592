"""Position gradients of the basis sums on the device (sph_convgrad.h) against the host twin, byte for byte, on the smallest shapes where
the kernel can go wrong (the scenes of test_gpu_conv); sentinels; the proof that a call changes neither the simulation nor a later
dispatch; the refusals; continuous_conv's positions= / points_grad= on the device; the example."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
from aggregate_ref import values_for
from conv_ref import planes_for, same
import query_scenes as QS
from support import build_example, linked_list_grid, run_example, slab_engine, undisturbed_run
from test_conv_posgrad_cpu import conv_bound, filters_for
from test_gpu_conv import combos, radii

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p


def check(pkg, f, rec, sp, size, what, pts=None, fluid_only=False, **kw):
    """Every combination (C, R, weight, SELF) of test_gpu_conv.combos against the host twin."""
    rows = len(rec) if pts is None else len(pts)
    for c, R, weight, self_ in combos(pkg, sp, size, **kw):
        args = dict(size=size, weight=weight, fluid_only=fluid_only)
        x, g = values_for(len(rec), c, seed=43), planes_for(rows, size, c)
        tag = f"{what} K {size} C {c} R {R:.3g} {weight} self {self_} fluid_only {fluid_only}"
        if pts is None:
            want = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, self_=self_, **args)
            assert want.any(), tag
            same(f.aggregate_basis_position_grad(x, g, R, self_=self_, **args), want, "particles " + tag)
        else:
            wp, wx = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, R, points=pts, **args)
            gp, gx = f.query_aggregate_basis_position_grad(pts, x, g, R, **args)
            assert wp.any() and wx.any(), tag
            same(gp, wp, "query points " + tag), same(gx, wx, "query particles " + tag)


@pytest.mark.parametrize("size", [2, 3, 4])
def test_uniform_every_channel_count(pkg, size):
    rec, sp = QS.uniform(pkg, 2001, 21)                                                 # (2001 rows: no multiple of the targets per block)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, size, "uniform")
    x, g = values_for(2001, 3), planes_for(2001, size, 3)
    for weight in ("one", "poly6"):                                                     # SELF moves no byte; weight "one" is not all zero
        a = f.aggregate_basis_position_grad(x, g, 1.0, size=size, weight=weight)
        same(f.aggregate_basis_position_grad(x, g, 1.0, size=size, weight=weight, self_=True), a, "SELF")
        assert a.any() and np.isfinite(a).all()
    f.close()


@pytest.mark.parametrize("size", [2, 3, 4])
def test_query_cloud(pkg, size):
    """Particles and points in clamped cells outside the grid, three non-finite points, 701 rows; both outputs and each alone."""
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, size, "query cloud", pts=pts, shift=1)
    x, g = values_for(n, 5), planes_for(m, size, 5)
    wp, wx = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, 1.0, points=pts, size=size)
    lo, dims, cs = QS.grid(pkg, sp)
    far = ((pts < lo) | (pts > lo + dims.astype(F) * cs)).any(axis=1)
    assert wp[far].any() and (wp[[5, 256, 700]].view(np.uint32) == 0).all()            # clamped cells take part; the non-finite points' rows are +0
    gp, none = f.query_aggregate_basis_position_grad(pts, x, g, 1.0, size=size, want_particles=False)
    assert none is None
    same(gp, wp, "points alone")
    none, gx = f.query_aggregate_basis_position_grad(pts, x, g, 1.0, size=size, want_points=False)
    assert none is None
    same(gx, wx, "particles alone")
    same(f.query_aggregate_basis_position_grad(pts, x, g, 1.0, size=size)[1], wx, "again")      # two calls in a row: the same bytes
    f.close()


def test_device_tensors_and_empty_calls(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    x, g, gn = values_for(n, 5), planes_for(m, 3, 5), planes_for(n, 3, 5)
    wp, wx = pkg.aggregate_basis_position_grad_host(rec, sp, x, g, 1.0, points=pts, size=3)
    # device tensors are used in place and never written
    p4 = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, np.ones((m, 1), F)], axis=1))).cuda()
    xt, gt, gnt = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(gn).cuda()
    dp, dx = f.query_aggregate_basis_position_grad(p4, xt, gt, 1.0, size=3, device=True)
    assert dp.is_cuda and tuple(dp.shape) == (m, 3) and tuple(dx.shape) == (n, 3)
    same(dp.cpu().numpy(), wp, "device tensors: points"), same(dx.cpu().numpy(), wx, "device tensors: particles")
    dn = f.aggregate_basis_position_grad(xt, gnt, 1.0, size=3, device=True)
    same(dn.cpu().numpy(), pkg.aggregate_basis_position_grad_host(rec, sp, x, gn, 1.0, size=3), "device tensors: particle targets")
    for t, a in ((xt, x), (gt, g), (gnt, gn)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
    # m = 0: the particles' output is zeroed; all points non-finite: +0 everywhere
    gp, gx = f.query_aggregate_basis_position_grad(np.zeros((0, 3), F), x, np.zeros((0, 27, 5), F), 1.0, size=3)
    assert gp.shape == (0, 3) and gx.shape == (n, 3) and (gx.view(np.uint32) == 0).all()
    bad = np.full((70, 3), np.nan, F)
    gp, gx = f.query_aggregate_basis_position_grad(bad, x, planes_for(70, 3, 5), 1.0, size=3)
    assert (gp.view(np.uint32) == 0).all() and (gx.view(np.uint32) == 0).all()
    f.close()
    empty = pkg.SPHFluidGPU.from_particles(np.zeros(0, pkg.PARTICLE_DTYPE), sp)         # n = 0: success, nothing to write
    assert empty.aggregate_basis_position_grad(np.zeros((0, 2), F), np.zeros((0, 8, 2), F), 1.0, size=2).shape == (0, 3)
    empty.close()


def test_crowded_cell_of_300(pkg):
    rec, sp, start, members = QS.crowded_cell(pkg, 300)
    assert members >= 300
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    pts = rec["pos"][::-1, :3].copy()                                                   # as many points in that cell
    for size, channels in ((4, (3, 65)), (3, (16,)), (2, (1, 64))):
        check(pkg, f, rec, sp, size, "crowd 300", channels=channels)
        check(pkg, f, rec, sp, size, "crowd 300", pts=pts, channels=channels[:1])
    f.close()


def test_lattice_coincident_and_ghosts(pkg):
    rec, sp = QS.lattice(pkg)                                                           # ties, offsets on cell boundaries of the filter grid
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for size in (2, 3, 4):
        check(pkg, f, rec, sp, size, "lattice", channels=(3, 16), shift=size)
    f.close()
    rec, sp, same_ = QS.coincident(pkg)                                                 # d = 0 pairs
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, 3, "coincident", channels=(3, 16, 65))
    check(pkg, f, rec, sp, 4, "coincident", pts=rec["pos"][::2, :3].copy(), channels=(5, 33))      # points on the particles
    f.close()
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fluid_only in (False, True):
        check(pkg, f, rec, sp, 4, "ghosts", channels=(5, 64), fluid_only=fluid_only)
        check(pkg, f, rec, sp, 2, "ghosts", pts=rec["pos"][:333, :3].copy(), channels=(3, 33), fluid_only=fluid_only)
    out = f.aggregate_basis_position_grad(values_for(len(rec), 5), planes_for(len(rec), 3, 5), 1.0, size=3, fluid_only=True)
    assert (out[ghost].view(np.uint32) == 0).all() and out[~ghost].any()                # a ghost's row is +0
    gx = f.query_aggregate_basis_position_grad(rec["pos"][:333, :3].copy(), values_for(len(rec), 5), planes_for(333, 3, 5), 1.0, size=3, fluid_only=True)[1]
    assert (gx[ghost].view(np.uint32) == 0).all() and gx[~ghost].any()
    f.close()
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, 3, "non-finite positions", channels=(5, 65))
    out = f.aggregate_basis_position_grad(values_for(1000, 5), planes_for(1000, 3, 5), 1.0, size=3)
    assert (out[[7, 300]].view(np.uint32) == 0).all() and np.isfinite(out).all()
    f.close()


def test_sentinels_info_and_the_staged_call(pkg):
    """Every row of the outputs and nothing beyond them is written; values, g and the points never."""
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    L = pkg.load_library()
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    pt = torch.from_numpy(p4).cuda()
    info = pkg.SphAggregateInfo()
    for c, size in ((5, 3), (65, 2), (16, 4)):
        x = torch.from_numpy(values_for(n, c)).cuda()
        gp, gq = torch.from_numpy(planes_for(n, size, c)).cuda(), torch.from_numpy(planes_for(m, size, c)).cuda()
        held = [t.clone() for t in (x, gp, gq, pt)]
        cfg = pkg.basis_config(radius=1.0, channels=c, size=size)
        a = torch.full((n * 3 + 64,), float("nan"), dtype=torch.float32, device="cuda")
        b = torch.full((m * 3 + 64,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert L.sph_aggregate_basis_posgrad_particles(f._h, C.byref(cfg), vp(x.data_ptr()), vp(gp.data_ptr()), vp(a.data_ptr() + 128), C.byref(info)) == 0
        f.sync()
        got = a.cpu().numpy()
        assert np.isnan(got[:32]).all() and np.isnan(got[32 + n * 3:]).all() and not np.isnan(got[32:32 + n * 3]).any()
        assert (info.rows, info.channels, info.planes, info.stencil, info.flags) == (n, c, size ** 3, 2, 0) and info.radius == 1.0
        a.fill_(float("nan"))
        torch.cuda.synchronize()
        assert L.sph_aggregate_basis_posgrad_query(f._h, C.byref(cfg), vp(pt.data_ptr()), m, vp(x.data_ptr()), vp(gq.data_ptr()), vp(b.data_ptr() + 128),
                                                   vp(a.data_ptr() + 128), C.byref(info)) == 0
        f.sync()
        for t, k in ((a, n), (b, m)):
            got = t.cpu().numpy()
            assert np.isnan(got[:32]).all() and np.isnan(got[32 + k * 3:]).all() and not np.isnan(got[32:32 + k * 3]).any()
        assert (info.rows, info.channels, info.planes) == (m, c, size ** 3)
        for t, h in zip((x, gp, gq, pt), held):
            assert torch.equal(t.view(torch.int32), h.view(torch.int32))
    # the staged call round-trips host arrays: the twin's bytes
    x, g, gq = values_for(n, 5), planes_for(n, 3, 5), planes_for(m, 3, 5)
    cfg = pkg.basis_config(radius=1.0, channels=5, size=3, flags=pkg.SPH_AGGREGATE_SELF)
    p = lambda arr: arr.ctypes.data_as(vp)
    out = np.full((n, 3), 7.0, F)
    assert L.sph_aggregate_basis_posgrad_staged(f._h, C.byref(cfg), None, 0, p(x), p(g), None, p(out), C.byref(info)) == 0
    same(out, pkg.aggregate_basis_position_grad_host(rec, sp, x, g, 1.0, size=3, self_=True), "staged, particles")
    cfg = pkg.basis_config(radius=1.0, channels=5, size=3)
    op, ox = np.full((m, 3), 7.0, F), np.full((n, 3), 7.0, F)
    assert L.sph_aggregate_basis_posgrad_staged(f._h, C.byref(cfg), p(p4), m, p(x), p(gq), p(op), p(ox), C.byref(info)) == 0
    wp, wx = pkg.aggregate_basis_position_grad_host(rec, sp, x, gq, 1.0, points=pts, size=3)
    same(op, wp, "staged, points"), same(ox, wx, "staged, query particles")
    f.close()


def test_refusals(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n, h = len(rec), sp.param_h
    x = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    g = torch.zeros((n, 8, 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    outp = torch.full((4, 3), 7.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    good = dict(radius=h, channels=4, size=2)
    p = lambda t: None if t is None else vp(t.data_ptr())

    def particles(e, cfg, x_=x, g_=g, out_=out):
        return L.sph_aggregate_basis_posgrad_particles(e, C.byref(cfg), p(x_), p(g_), p(out_), C.byref(info))

    def query(e, cfg, m=4, pts_=pts, outp_=outp, out_=out):
        return L.sph_aggregate_basis_posgrad_query(e, C.byref(cfg), p(pts_), m, p(x), p(g), p(outp_), p(out_), C.byref(info))

    with slab_engine(pkg, rec, sp) as slab:
        assert particles(slab._h, pkg.basis_config(**good)) == -3 and b"slab" in L.sph_last_error()
        assert query(slab._h, pkg.basis_config(**good)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        assert particles(f._h, pkg.basis_config(**good)) == -3 and query(f._h, pkg.basis_config(**good)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.aggregate_basis_position_grad(x, g, size=2)
    assert particles(None, pkg.basis_config(**good)) == -1 and particles(f._h, pkg.basis_config(**good), x_=None) == -1
    assert particles(f._h, pkg.basis_config(**good), g_=None) == -1 and particles(f._h, pkg.basis_config(**good), out_=None) == -1
    assert query(f._h, pkg.basis_config(**good), outp_=None, out_=None) == -1           # both outputs null
    assert query(f._h, pkg.basis_config(**good), pts_=None) == -1
    for bad in (dict(weight=2), dict(flags=pkg.SPH_AGGREGATE_DELTA), dict(flags=pkg.SPH_AGGREGATE_MOMENTS), dict(flags=16), dict(channels=0), dict(channels=129),
                dict(kind=1), dict(size=1), dict(size=5), dict(radius=0.0), dict(radius=3.01 * h)):
        assert particles(f._h, pkg.basis_config(**dict(good, **bad))) == -1, bad
        assert query(f._h, pkg.basis_config(**dict(good, **bad))) == -1, bad
    assert query(f._h, pkg.basis_config(flags=pkg.SPH_AGGREGATE_SELF, **good)) == -1
    assert query(f._h, pkg.basis_config(**good), m=1 << 31) == -1
    flat = g.view(-1)
    assert particles(f._h, pkg.basis_config(**good), g_=flat, out_=flat[n * 32 - 4:]) == -1 and b"overlap" in L.sph_last_error()
    assert particles(f._h, pkg.basis_config(**good), x_=flat, out_=flat[8:]) == -1
    assert query(f._h, pkg.basis_config(**good), outp_=flat[4:], out_=flat) == -1       # the outputs overlap each other (and g)
    assert query(f._h, pkg.basis_config(**good), outp_=out.view(-1)[4:], out_=out) == -1
    assert query(f._h, pkg.basis_config(**good), pts_=flat, outp_=flat[8:]) == -1
    f.sync()
    assert (out == 7.0).all().item() and (outp == 7.0).all().item() and (g == 0).all().item()   # no refused call wrote anything
    assert particles(f._h, pkg.basis_config(**good)) == 0                                       # ... and the valid call works afterwards
    f.sync()
    assert (out == 0.0).all().item()
    f.close()


def test_a_call_does_not_change_the_simulation(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n = len(rec)
    pts = rec["pos"][::5, :3].copy()
    x, g, gq = values_for(n, 5), planes_for(n, 3, 5), planes_for(len(pts), 3, 5)
    filt = torch.from_numpy(filters_for(3, 5, 2)).cuda()

    def probe(f):
        f.aggregate_basis_position_grad(x, g, 2.0 * sp.param_h, size=3, self_=True)
        f.query_aggregate_basis_position_grad(pts, x, gq, sp.param_h, size=3, weight="one")
        xt, pt = torch.from_numpy(x).cuda().requires_grad_(True), f.positions(device=True).requires_grad_(True)
        f.continuous_conv(xt, filt, positions=pt, normalize=True).sum().backward()

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
    R = radii(pkg, sp)[1]
    pos = f.positions(device=True)
    gen = torch.Generator().manual_seed(6)
    # one block, no normalize: positions.grad is the direct call, byte for byte; x.grad and filters.grad the bytes without the keyword
    for K, cin, cout, weight, self_ in ((3, 16, 8, "poly6", True), (4, 5, 3, "one", False)):
        xv, fv = torch.randn((n, cin), generator=gen).cuda(), (torch.randn((K, K, K, cin, cout), generator=gen) / K ** 3).cuda()
        g = torch.randn((n, cout), generator=gen).cuda()
        x, filt, pt = xv.clone().requires_grad_(True), fv.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        y = f.continuous_conv(x, filt, R, weight=weight, self_=self_, positions=pt)
        y.backward(g)
        x2, filt2 = xv.clone().requires_grad_(True), fv.clone().requires_grad_(True)
        y2 = f.continuous_conv(x2, filt2, R, weight=weight, self_=self_)
        y2.backward(g)
        for a, b, what in ((y, y2, "out"), (x.grad, x2.grad, "x.grad"), (filt.grad, filt2.grad, "filters.grad")):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), what
        h = (g @ fv.reshape(-1, cout).t()).reshape(n, K ** 3, cin).contiguous()
        direct = f.aggregate_basis_position_grad(xv, h, R, size=K, weight=weight, self_=self_)
        same(pt.grad.cpu().numpy(), direct, f"positions.grad K {K}")
        same(direct, pkg.aggregate_basis_position_grad_host(rec, sp, xv.cpu().numpy(), h.cpu().numpy(), R, size=K, weight=weight, self_=self_), "the twin of that h")
    # normalize: within the CPU test's bound of the host backend (torch's matrix products and elementwise kernels sit between the calls)
    K, cin, cout = 3, 5, 4
    xv, fv, g = values_for(n, cin, seed=55), filters_for(K, cin, cout), values_for(n, cout, seed=58)
    x, filt, pt = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (xv, fv, pos.cpu().numpy()))
    y = f.continuous_conv(x, filt, R, normalize=True, positions=pt)
    (y * torch.from_numpy(g).cuda()).sum().backward()
    host = pkg.HostAggregateBackend(rec, sp)
    xh, fh, ph = torch.from_numpy(xv).requires_grad_(True), torch.from_numpy(fv).requires_grad_(True), host.positions().requires_grad_(True)
    yh = pkg.continuous_conv(host, None, xh, fh, R, normalize=True, positions=ph)
    (yh * torch.from_numpy(g)).sum().backward()
    _, bound = conv_bound(pkg, rec, sp, xv, g, yh.detach().numpy().astype(np.float64), fv, R, [(0, cin)], self_=True, normalize=True)
    got, want = pt.grad.cpu().numpy(), ph.grad.numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"normalize: largest |gradient| {np.abs(want).max():.4g}, largest device - host {err.max():.3g}, largest over bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.abs(want).max() > 0 and (err <= bound).all()
    # a positions tensor that is not the engine's raises
    moved = pos.clone()
    moved[17, 1] += 1e-3
    with pytest.raises(pkg.SphError, match="positions"):
        f.continuous_conv(x.detach(), filt.detach(), R, positions=moved.requires_grad_(True))
    # query targets: points.grad and positions.grad are the direct call's two outputs
    rec2, sp2, pts = QS.query_cloud(pkg)
    f2 = pkg.SPHFluidGPU.from_particles(rec2, sp2)
    n2, m = len(rec2), len(pts)
    xv, fv = torch.randn((n2, 3), generator=gen).cuda(), (torch.randn((4, 4, 4, 3, 2), generator=gen) / 64).cuda()
    g = torch.randn((m, 2), generator=gen).cuda()
    h = (g @ fv.reshape(-1, 2).t()).reshape(m, 64, 3).contiguous()
    wp, wx = f2.query_aggregate_basis_position_grad(pts, xv, h, 1.0, size=4)
    for width in (3, 4):
        x, filt2, pt = xv.clone().requires_grad_(True), fv.clone().requires_grad_(True), f2.positions(device=True).requires_grad_(True)
        full = pts if width == 3 else np.concatenate([pts, np.ones((m, 1), F)], axis=1)
        qt = torch.from_numpy(np.ascontiguousarray(full)).cuda().requires_grad_(True)
        y = f2.query_continuous_conv(qt, x, filt2, 1.0, positions=pt, points_grad=True)
        y.backward(g)
        same(qt.grad.cpu().numpy()[:, :3].copy(), wp, f"points.grad, width {width}")
        same(pt.grad.cpu().numpy(), wx, "positions.grad")
        assert tuple(qt.grad.shape) == (m, width) and not qt.grad[:, 3:].any().item()
    f2.close()
    # a dispatch between forward and backward raises
    x, pt = torch.from_numpy(values_for(n, cin, seed=55)).cuda().requires_grad_(True), pos.clone().requires_grad_(True)
    y = f.continuous_conv(x, filt.detach(), R, positions=pt)
    f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    f.close()


def test_conv_position_gradient_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "conv_position_gradient", tmp_path, werror=True), ["20000"], timeout=120)
    assert res.returncode == 0 and "conv_position_gradient OK" in res.stdout
