"""The filter-grid basis sums, their adjoint and continuous_conv on the device (sph_conv.h) against the host twins, byte for byte, on the
smallest shapes where the device code can go wrong: groups that are not filled, exactly one wave, a second pass over the candidates
and the channel cap; every filter size and stencil; the crowded cell, empty rows, row counts that are no multiple of the targets per
block, empty calls, points outside the grid and non-finite points; repeatability; sentinels; the proof that a call changes neither the
simulation nor the state digest; the C++ twin."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
from aggregate_ref import values_for
import conv_ref as CR
from conv_ref import same
import query_scenes as QS
from support import build_example, linked_list_grid, run_example, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
CHANNELS = (1, 3, 16, 33, 64, 65, 128)     # a group not filled, a full group, exactly one wave, a second pass, the cap


def radii(pkg, sp):
    """0.7 h, h and 2.5 cells: the three stencil half-widths."""
    h, cs = F(sp.param_h), QS.grid(pkg, sp)[2]
    return float(F(0.7) * h), float(h), float(F(2.5) * cs)


def combos(pkg, sp, size, shift=0, channels=CHANNELS):
    """(C, R, weight, self_) for one filter size: every channel count, the radii, weights and SELF rotating."""
    R = radii(pkg, sp)
    return [(c, R[(i + size + shift) % 3], ("one", "poly6")[(i + shift) % 2], bool((i + size + shift) % 2)) for i, c in enumerate(channels)]


def check(pkg, f, rec, sp, size, what, pts=None, fluid_only=False, **kw):
    """Forward (with counts) and adjoint of every combination against the host twins."""
    rows = len(rec) if pts is None else len(pts)
    for c, R, weight, self_ in combos(pkg, sp, size, **kw):
        args = dict(size=size, weight=weight, fluid_only=fluid_only)
        if pts is None:
            args["self_"] = self_
        x, h = values_for(len(rec), c), CR.planes_for(rows, size, c)
        tag = f"{what} K {size} C {c} R {R:.3f} {args}"
        if pts is None:
            got, cnt = f.aggregate_basis(x, R, counts=True, **args)
            adj = f.aggregate_basis_adjoint(h, R, **args)
        else:
            got, cnt = f.query_aggregate_basis(pts, x, R, counts=True, **args)
            adj = f.query_aggregate_basis_adjoint(pts, h, R, **args)
        want, wcnt = pkg.aggregate_basis_host(rec, sp, x, R, points=pts, counts=True, **args)
        same(got, want, "forward " + tag), same(cnt, wcnt, "counts " + tag)
        same(adj, pkg.aggregate_basis_adjoint_host(rec, sp, h, R, points=pts, **args), "adjoint " + tag)


@pytest.mark.parametrize("size", [2, 3, 4])
def test_uniform_every_channel_count(pkg, size):
    rec, sp = QS.uniform(pkg, 2001, 21)                                                 # (2001 rows: no multiple of the targets per block)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, size, "uniform")
    x = values_for(len(rec), 3)
    out, cnt = f.aggregate_basis(x, radii(pkg, sp)[0], size=size, counts=True)
    assert (cnt == 0).any() and not out[cnt == 0].any() and not np.signbit(out[cnt == 0]).any()     # a target with no neighbour: +0
    f.close()


@pytest.mark.parametrize("size", [2, 3, 4])
def test_query_cloud(pkg, size):
    """Particles and points in clamped cells outside the grid, three non-finite points, 701 rows."""
    rec, sp, pts = QS.query_cloud(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, size, "query cloud", pts=pts, shift=1)
    check(pkg, f, rec, sp, size, "query cloud, particles", shift=2, channels=(3, 33, 65))
    x = values_for(len(rec), 3)
    out, cnt = f.query_aggregate_basis(pts, x, radii(pkg, sp)[2], size=size, counts=True)
    gone = [5, 256, 700]
    assert (cnt[gone] == 0).all() and (out[gone].view(np.uint32) == 0).all() and cnt.sum() > 0
    h = CR.planes_for(len(pts), size, 3)
    h2 = h.copy()
    h2[gone] = 1000.0                                                                   # what a non-finite point carries reaches nobody
    same(f.query_aggregate_basis_adjoint(pts, h2, 1.0, size=size), f.query_aggregate_basis_adjoint(pts, h, 1.0, size=size), "non-finite points")
    f.close()


def test_crowded_cell_of_300(pkg):
    rec, sp, start, members = QS.crowded_cell(pkg, 300)
    assert members >= 300
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for size, channels in ((4, (3, 65)), (3, (16, 128)), (2, (1, 64))):
        check(pkg, f, rec, sp, size, "crowd 300", channels=channels)
        check(pkg, f, rec, sp, size, "crowd 300, as many points in that cell", pts=rec["pos"][::-1, :3].copy(), channels=channels[:1])
    f.close()


def test_coincident_ghosts_and_non_finite_positions(pkg):
    rec, sp, same_ = QS.coincident(pkg, n=2000)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, 3, "coincident", channels=(3, 16, 65))
    f.close()
    rec, sp = QS.with_ghosts(pkg, n=2400)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fluid_only in (False, True):
        check(pkg, f, rec, sp, 4, "ghosts", channels=(1, 33, 128), fluid_only=fluid_only)
        check(pkg, f, rec, sp, 2, "ghosts, query", pts=rec["pos"][:333, :3].copy(), channels=(3, 64), fluid_only=fluid_only)
    out = f.aggregate_basis(values_for(len(rec), 3), 1.0, size=3, self_=True, fluid_only=True)
    adj = f.aggregate_basis_adjoint(CR.planes_for(len(rec), 3, 3), 1.0, size=3, self_=True, fluid_only=True)
    assert (out[ghost].view(np.uint32) == 0).all() and (adj[ghost].view(np.uint32) == 0).all() and out[~ghost].any() and adj[~ghost].any()
    f.close()
    rec, sp = QS.uniform(pkg, 2000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    check(pkg, f, rec, sp, 3, "non-finite positions", channels=(3, 33))
    x = values_for(len(rec), 3)
    out = f.aggregate_basis(x, 1.0, size=3, weight="one", self_=True)
    assert np.array_equal(out[[7, 300], 13], x[[7, 300]]) and not np.delete(out[[7, 300]], 13, axis=1).any()     # the own slot alone, in the centre cell
    f.close()


def test_empty_calls(pkg):
    rec, sp = QS.uniform(pkg, 500, 21)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    none3 = np.zeros((0, 3), F)
    out, cnt = f.query_aggregate_basis(none3, values_for(500, 5), 1.0, size=3, counts=True)
    assert out.shape == (0, 27, 5) and cnt.shape == (0,)
    adj = f.query_aggregate_basis_adjoint(none3, np.zeros((0, 27, 5), F), 1.0, size=3)
    assert adj.shape == (500, 5) and (adj.view(np.uint32) == 0).all()                    # m = 0: out is zeroed
    bad = np.full((70, 3), np.nan, F)
    bad[1::2] = np.inf
    adj = f.query_aggregate_basis_adjoint(bad, CR.planes_for(70, 2, 3), 1.0, size=2)
    assert adj.shape == (500, 3) and (adj.view(np.uint32) == 0).all()                    # all points non-finite: +0 everywhere
    f.close()
    f = pkg.SPHFluidGPU.from_particles(np.zeros(0, pkg.PARTICLE_DTYPE), sp)              # n = 0
    assert f.aggregate_basis(np.zeros((0, 4), F), 1.0, size=4).shape == (0, 64, 4)
    out = f.query_aggregate_basis(rec["pos"][:9, :3].copy(), np.zeros((0, 4), F), 1.0, size=2)
    assert out.shape == (9, 8, 4) and not out.any()
    assert f.aggregate_basis_adjoint(np.zeros((0, 8, 2), F), 1.0, size=2).shape == (0, 2)
    assert f.query_aggregate_basis_adjoint(rec["pos"][:9, :3].copy(), np.zeros((9, 8, 2), F), 1.0, size=2).shape == (0, 2)
    f.close()


def test_repeatable_and_the_same_from_a_second_engine(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    f, f2 = pkg.SPHFluidGPU.from_particles(rec, sp), pkg.SPHFluidGPU.from_particles(rec, sp)
    R = radii(pkg, sp)[2]
    for c, size in ((3, 4), (65, 3)):
        x, hp, hq = values_for(len(rec), c), CR.planes_for(len(rec), size, c), CR.planes_for(len(pts), size, c)
        calls = (lambda e: e.aggregate_basis(x, R, size=size, self_=True), lambda e: e.query_aggregate_basis(pts, x, R, size=size),
                 lambda e: e.aggregate_basis_adjoint(hp, R, size=size, self_=True), lambda e: e.query_aggregate_basis_adjoint(pts, hq, R, size=size))
        for i, call in enumerate(calls):
            first = call(f)
            assert first.any()
            same(call(f), first, f"call {i}, two in a row"), same(call(f2), first, f"call {i}, a second engine")
    f.close(), f2.close()


def test_sentinels(pkg):
    """Every row of out and nothing beyond it is written; the inputs never."""
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
        B = size ** 3
        cfg = pkg.basis_config(radius=1.0, channels=c, size=size)
        x = torch.from_numpy(values_for(n, c)).cuda()
        hp, hq = torch.from_numpy(CR.planes_for(n, size, c)).cuda(), torch.from_numpy(CR.planes_for(m, size, c)).cuda()
        held = [t.clone() for t in (x, hp, hq, pt)]
        calls = {
            "forward, particles": (n * B * c, n, lambda o, k: L.sph_aggregate_basis_particles(f._h, C.byref(cfg), vp(x.data_ptr()), o, k, C.byref(info))),
            "forward, query": (m * B * c, m, lambda o, k: L.sph_aggregate_basis_query(f._h, C.byref(cfg), vp(pt.data_ptr()), m, vp(x.data_ptr()), o, k, C.byref(info))),
            "adjoint, particles": (n * c, 0, lambda o, k: L.sph_aggregate_basis_adjoint_particles(f._h, C.byref(cfg), vp(hp.data_ptr()), o, C.byref(info))),
            "adjoint, query": (n * c, 0, lambda o, k: L.sph_aggregate_basis_adjoint_query(f._h, C.byref(cfg), vp(pt.data_ptr()), m, vp(hq.data_ptr()), o, C.byref(info))),
        }
        for name, (words, rows, call) in calls.items():
            buf = torch.full((words + 64,), float("nan"), dtype=torch.float32, device="cuda")
            cnt = torch.full((rows + 64,), 2 ** 31 - 1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert call(vp(buf.data_ptr() + 128), vp(cnt.data_ptr() + 128)) == 0, name
            f.sync()
            got, k = buf.cpu().numpy(), cnt.cpu().numpy()
            assert np.isnan(got[:32]).all() and np.isnan(got[32 + words:]).all() and not np.isnan(got[32:32 + words]).any(), name
            assert (k[:32] == 2 ** 31 - 1).all() and (k[32 + rows:] == 2 ** 31 - 1).all() and (rows == 0 or (k[32:32 + rows] < n + 1).all()), name
            assert (info.channels, info.planes, info.stencil) == (c, B, 2) and info.rows == (m if name == "forward, query" else n), name
        for t, h in zip((x, hp, hq, pt), held):
            assert torch.equal(t.view(torch.int32), h.view(torch.int32))
    f.close()


def test_refusals(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n, h = len(rec), sp.param_h
    x = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    big = torch.full((n, 8, 4), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    good = dict(radius=h, channels=4, size=2)
    p = lambda t: None if t is None else vp(t.data_ptr())

    def forward(e, cfg, x_=x, out_=big):
        return L.sph_aggregate_basis_particles(e, C.byref(cfg), p(x_), p(out_), None, C.byref(info))

    def forward_query(e, cfg, m=4):
        return L.sph_aggregate_basis_query(e, C.byref(cfg), p(pts), m, p(x), p(big), None, C.byref(info))

    def adjoint(e, cfg, h_=big, out_=out):
        return L.sph_aggregate_basis_adjoint_particles(e, C.byref(cfg), p(h_), p(out_), C.byref(info))

    def adjoint_query(e, cfg, m=4):
        return L.sph_aggregate_basis_adjoint_query(e, C.byref(cfg), p(pts), m, p(big), p(out), C.byref(info))

    every = (forward, forward_query, adjoint, adjoint_query)
    with slab_engine(pkg, rec, sp) as slab:
        assert all(call(slab._h, pkg.basis_config(**good)) == -3 for call in every) and b"slab" in L.sph_last_error()
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        assert all(call(f._h, pkg.basis_config(**good)) == -3 for call in every)
        with pytest.raises(pkg.SphError, match="-3"):
            f.aggregate_basis(x, size=2)
    assert forward(None, pkg.basis_config(**good)) == -1 and forward(f._h, pkg.basis_config(**good), x_=None) == -1
    assert forward(f._h, pkg.basis_config(**good), out_=None) == -1 and adjoint(f._h, pkg.basis_config(**good), h_=None) == -1
    assert adjoint(f._h, pkg.basis_config(**good), out_=None) == -1
    for bad in (dict(weight=2), dict(flags=pkg.SPH_AGGREGATE_DELTA), dict(flags=pkg.SPH_AGGREGATE_MOMENTS), dict(flags=16), dict(channels=0), dict(channels=129),
                dict(kind=1), dict(size=1), dict(size=5), dict(radius=0.0), dict(radius=3.01 * h)):
        assert all(call(f._h, pkg.basis_config(**dict(good, **bad))) == -1 for call in every), bad
    assert forward_query(f._h, pkg.basis_config(flags=pkg.SPH_AGGREGATE_SELF, **good)) == -1
    assert adjoint_query(f._h, pkg.basis_config(flags=pkg.SPH_AGGREGATE_SELF, **good)) == -1
    assert forward_query(f._h, pkg.basis_config(**good), m=1 << 31) == -1 and adjoint_query(f._h, pkg.basis_config(**good), m=1 << 31) == -1
    flat = big.view(-1)
    assert forward(f._h, pkg.basis_config(**good), x_=flat[n * 32 - 8:], out_=big) == -1 and b"overlap" in L.sph_last_error()
    assert adjoint(f._h, pkg.basis_config(**good), h_=big, out_=flat[n * 32 - 8:]) == -1 and b"overlap" in L.sph_last_error()
    f.sync()
    assert (big == 7.0).all().item() and (out == 7.0).all().item() and (x == 0).all().item()     # no refused call wrote anything
    assert forward(f._h, pkg.basis_config(**good)) == 0                                          # ... and the valid calls work afterwards
    f.sync()
    assert (big == 0.0).all().item()
    assert adjoint(f._h, pkg.basis_config(**good)) == 0
    f.sync()
    assert (out == 0.0).all().item()
    f.close()


def blocked_product(A_of, x, filt, blocks):
    """continuous_conv's forward as the docstring states it: per block of input channels one product, the first assigned, the rest added."""
    out = None
    for c0, c1 in blocks:
        A = A_of(x[:, c0:c1].contiguous())
        part = A.reshape(A.shape[0], -1) @ filt[:, :, :, c0:c1, :].reshape(-1, filt.shape[4])
        out = part if out is None else out + part
    return out


def test_continuous_conv_on_the_device(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    n, m = len(rec), len(pts)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    R = radii(pkg, sp)[1]
    gen = torch.Generator().manual_seed(5)
    for K, cin, cout, blocks, limit in ((3, 16, 8, [(0, 16)], 2 ** 31), (4, 7, 5, [(0, 3), (3, 6), (6, 7)], n * 64 * 4 * 3), (2, 33, 3, [(0, 33)], 2 ** 31)):
        B = K ** 3
        xv, fv = torch.randn((n, cin), generator=gen).cuda(), (torch.randn((K, K, K, cin, cout), generator=gen) / B).cuda()
        x, filt = xv.clone().requires_grad_(True), fv.clone().requires_grad_(True)
        y = f.continuous_conv(x, filt, R, max_basis_bytes=limit)
        assert y.is_cuda and tuple(y.shape) == (n, cout) and y.requires_grad
        want = blocked_product(lambda xb: f.aggregate_basis(xb, R, size=K, self_=True, device=True), xv, fv, blocks)
        assert torch.equal(y.detach().view(torch.int32), want.view(torch.int32)), f"forward K {K}: the same products of the same bytes"
        g = torch.randn((n, cout), generator=gen).cuda()
        y.backward(g)
        for c0, c1 in blocks:
            h = (g @ fv[:, :, :, c0:c1, :].reshape(-1, cout).t()).reshape(n, B, c1 - c0).contiguous()
            gx = f.aggregate_basis_adjoint(h, R, size=K, self_=True, device=True)
            assert torch.equal(x.grad[:, c0:c1].contiguous().view(torch.int32), gx.view(torch.int32)), f"x.grad K {K} block {c0}"
            same(gx.cpu().numpy(), pkg.aggregate_basis_adjoint_host(rec, sp, h.cpu().numpy(), R, size=K, self_=True), "the adjoint of that h on the host")
            A = f.aggregate_basis(xv[:, c0:c1].contiguous(), R, size=K, self_=True, device=True)
            gf = (A.reshape(n, -1).t() @ g).reshape(K, K, K, c1 - c0, cout)
            assert torch.equal(filt.grad[:, :, :, c0:c1, :].contiguous().view(torch.int32), gf.contiguous().view(torch.int32)), f"filters.grad K {K} block {c0}"
    # query targets with normalize, against the host backend (the matrix products differ between the two: a tolerance, not bytes)
    xv, fv = torch.randn((n, 5), generator=gen), torch.randn((3, 3, 3, 5, 4), generator=gen) / 27
    x, filt = xv.cuda().requires_grad_(True), fv.cuda().requires_grad_(True)
    y = f.query_continuous_conv(pts, x, filt, R, normalize=True)
    g = torch.randn((m, 4), generator=gen)
    y.backward(g.cuda())
    xh, fh = xv.clone().requires_grad_(True), fv.clone().requires_grad_(True)
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = pts
    yh = pkg.continuous_conv(pkg.HostAggregateBackend(rec, sp), p4, xh, fh, R, self_=False, normalize=True)
    yh.backward(g)
    assert torch.allclose(y.detach().cpu(), yh.detach(), rtol=1e-4, atol=1e-5) and torch.allclose(x.grad.cpu(), xh.grad, rtol=1e-4, atol=1e-5)
    assert torch.allclose(filt.grad.cpu(), fh.grad, rtol=1e-4, atol=1e-4) and not y[[5, 256, 700]].any().item()
    # a dispatch between forward and backward
    x = xv.cuda().requires_grad_(True)
    y = f.continuous_conv(x, fv.cuda(), R)
    f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    x = xv.cuda().requires_grad_(True)
    y = f.continuous_conv(x, fv.cuda(), R, check_state=False)
    f.DispatchCompute()
    y.sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (n, 5)
    f.close()


def test_calls_do_not_change_the_simulation(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n = len(rec)
    pts = rec["pos"][::5, :3].copy()
    x, hp, hq = values_for(n, 5), CR.planes_for(n, 3, 5), CR.planes_for(len(pts), 3, 5)
    filt = torch.from_numpy(np.random.default_rng(4).normal(0.0, 0.1, (3, 3, 3, 5, 2)).astype(F)).cuda()

    def probe(f):
        f.aggregate_basis(x, size=3, self_=True)
        f.query_aggregate_basis(pts, x, 2.0 * sp.param_h, size=3)
        f.aggregate_basis_adjoint(hp, size=3)
        f.query_aggregate_basis_adjoint(pts, hq, sp.param_h, size=3, weight="one")
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        f.continuous_conv(xt, filt).sum().backward()

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchCompute()
    before = f.state_digest()
    probe(f)
    assert f.state_digest() == before                                                   # nothing of a call is engine state
    f.close()


def test_continuous_conv_example_and_the_twin_bytes(pkg, tmp_path):
    """The C++ twin: one call of each method from examples/continuous_conv.cpp; what it wrote against Python's host twins of the same inputs."""
    dump = tmp_path / "conv.bin"
    res = run_example(build_example(pkg, "continuous_conv", tmp_path, werror=True), ["6000", str(dump)], timeout=120)
    assert res.returncode == 0 and "continuous_conv OK" in res.stdout
    raw = dump.read_bytes()
    n, m, c, K = (int(v) for v in np.frombuffer(raw, np.uint64, 4))
    at = 32
    sp = pkg.SphParams.from_buffer_copy(raw[at:at + C.sizeof(pkg.SphParams)])
    at += C.sizeof(pkg.SphParams)

    def take(dtype, count, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at).reshape(shape).copy()
        at += a.nbytes
        return a

    B = K ** 3
    rec, vel, pts = take(pkg.PARTICLE_DTYPE, n, (n,)), take(F, n * c, (n, c)), take(F, m * 4, (m, 4))
    around, lattice, back, back_q = take(F, n * B * c, (n, B, c)), take(F, m * B * c, (m, B, c)), take(F, n * c, (n, c)), take(F, n * c, (n, c))
    assert at == len(raw) and around.any() and lattice.any()
    R = 2.0 * sp.param_h
    same(around, pkg.aggregate_basis_host(rec, sp, vel, R, size=K, self_=True), "AggregateBasis")
    same(lattice, pkg.aggregate_basis_host(rec, sp, vel, R, points=pts, size=K), "AggregateBasis, query points")
    same(back, pkg.aggregate_basis_adjoint_host(rec, sp, around, R, size=K, self_=True), "AggregateBasisAdjoint")
    same(back_q, pkg.aggregate_basis_adjoint_host(rec, sp, lattice, R, points=pts, size=K), "AggregateBasisAdjoint, query points")
