"""The fused neighbourhood reductions on the device (sph_aggregate.h) against sph_aggregate_host, byte for byte, in every variant of
SPH_OPT_AGGREGATE_VARIANT (staged / gathered by id, 4 / 8 / 16 channels per pass, 16-byte / 4-byte loads), on the smallest shapes where
they can go wrong; the interface around them; and the proof that a call changes neither the simulation nor a later dispatch."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import aggregate_ref as AR
from aggregate_ref import PARTICLE_CASES, QUERY_CASES, radius_of, same_bytes, values_for
import query_scenes as QS
from support import after_dispatches, build_example, linked_list_grid, records, run_example, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
# SPH_OPT_AGGREGATE_VARIANT: the default, the gather by id, each chunk width in both, 4-byte loads
VARIANTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
FEW = (0, 1, 6, 8)


def _same(pkg, f, rec, sp, case, what, points=None, variants=VARIANTS, **kw):
    """Every variant gives sph_aggregate_host's bytes; returns the host result."""
    op, weight, self_, delta, moments, fac, c = case
    x = values_for(len(rec), c)
    R = radius_of(sp, fac)
    args = dict(op=op, weight=weight, moments=moments, **kw)
    if points is None:
        args.update(self_=self_, delta=delta)
    want = pkg.aggregate_host(rec, sp, x, R, points=points, counts=True, **args)
    for variant in variants:
        f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, variant)
        got = f.aggregate(x, R, counts=True, **args) if points is None else f.query_aggregate(points, x, R, counts=True, **args)
        same_bytes(got, want, f"{what} {args} R {fac} h C {c} variant {variant}")
    f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, 0)
    return want


def test_uniform_every_case_and_variant(pkg):
    rec, sp = QS.uniform(pkg, 1000, 21)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in PARTICLE_CASES:
        _same(pkg, f, rec, sp, case, "uniform")
    f.close()


@pytest.mark.parametrize("crowd", [65, 200])
def test_crowded_cell(pkg, crowd):
    rec, sp, start, members = QS.crowded_cell(pkg, crowd)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in PARTICLE_CASES:
        _same(pkg, f, rec, sp, case, f"crowd {crowd}", variants=FEW)
    f.close()


def test_ties_coincident_ghosts_and_non_finite(pkg):
    rec, sp = QS.lattice(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in PARTICLE_CASES[::2]:
        _same(pkg, f, rec, sp, case, "lattice", variants=FEW)
    f.close()
    rec, sp, same = QS.coincident(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in PARTICLE_CASES[1::2]:
        _same(pkg, f, rec, sp, case, "coincident", variants=FEW)
    f.close()
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fluid_only in (False, True):
        for case in PARTICLE_CASES[::3]:
            out, cnt = _same(pkg, f, rec, sp, case, "ghosts", variants=FEW, fluid_only=fluid_only)
            assert not fluid_only or (cnt[ghost] == 0).all()
        _same(pkg, f, rec, sp, QUERY_CASES[1], "ghosts, query", points=rec["pos"][:333, :3], variants=FEW, fluid_only=fluid_only)
    f.close()
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in PARTICLE_CASES[4:8]:
        _same(pkg, f, rec, sp, case, "non-finite positions", variants=FEW)
    x = values_for(len(rec), 4)
    x[11, 0], x[12, 1], x[13, 2] = np.nan, np.inf, -0.0
    for op, weight in (("sum", "one"), ("mean", "poly6"), ("max", "one"), ("min", "one")):
        want = pkg.aggregate_host(rec, sp, x, 1.0, op=op, weight=weight, counts=True)
        same_bytes(f.aggregate(x, 1.0, op=op, weight=weight, counts=True), want, f"NaN / inf values, {op}")
    f.close()


def test_query_rows(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for case in QUERY_CASES:
        out, cnt = _same(pkg, f, rec, sp, case, "query", points=pts, variants=FEW)
        assert cnt[5] == 0 and cnt[256] == 0 and cnt[700] == 0 and cnt.sum() > 0
    # a torch device tensor of (m, 4) is used in place; the particles' own positions as queries are the SELF rows
    p4 = torch.from_numpy(np.ascontiguousarray(rec["pos"])).cuda()
    x = values_for(len(rec), 5)
    q = f.query_aggregate(p4, x, 1.0, op="mean", weight="poly6", counts=True)
    same_bytes(q, pkg.aggregate_host(rec, sp, x, 1.0, op="mean", weight="poly6", self_=True, counts=True), "positions as queries")
    f.close()


def test_numpy_and_torch_values_and_sentinels(pkg):
    """numpy values (uploaded) and a torch device tensor (used in place) give the same bytes; with device=True the results are torch
    tensors; a sentinel around the output shows that every row and nothing beyond rows * planes * C is written, and the values never."""
    import torch
    rec, sp = QS.uniform(pkg, 1000, 21)
    n = len(rec)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    L = pkg.load_library()
    for c, moments in ((5, True), (16, False), (1, False)):
        x = values_for(n, c)
        want = pkg.aggregate_host(rec, sp, x, 1.0, delta=True, moments=moments, counts=True)
        xt = torch.from_numpy(x).cuda()
        same_bytes(f.aggregate(x, 1.0, delta=True, moments=moments, counts=True), want, "numpy values")
        same_bytes(f.aggregate(xt, 1.0, delta=True, moments=moments, counts=True), want, "torch values in place")
        out, cnt = f.aggregate(xt, 1.0, delta=True, moments=moments, counts=True, device=True)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == want[0].shape and cnt.dtype == torch.int32
        same_bytes((out.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)), want, "device results")
        assert np.array_equal(xt.cpu().numpy().view(np.uint32), x.view(np.uint32))
        planes = 4 if moments else 1
        words = n * planes * c
        for variant in FEW:
            f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, variant)
            buf = torch.full((words + 64,), 12345.0, dtype=torch.float32, device="cuda")
            cbuf = torch.full((n + 64,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            cfg = pkg.aggregate_config(radius=1.0, channels=c, flags=pkg.SPH_AGGREGATE_DELTA | (pkg.SPH_AGGREGATE_MOMENTS if moments else 0))
            info = pkg.SphAggregateInfo()
            assert L.sph_aggregate_particles(f._h, C.byref(cfg), vp(xt.data_ptr()), vp(buf.data_ptr() + 128), vp(cbuf.data_ptr() + 128), C.byref(info)) == 0
            f.sync()
            assert (info.rows, info.channels, info.planes, info.stencil, info.flags) == (n, c, planes, 2, cfg.flags) and info.radius == 1.0
            got, gcnt = buf.cpu().numpy(), cbuf.cpu().numpy()
            assert (got[:32] == 12345.0).all() and (got[32 + words:] == 12345.0).all() and (gcnt[:32] == 77).all() and (gcnt[32 + n:] == 77).all()
            same_bytes((got[32:32 + words].reshape(want[0].shape), gcnt[32:32 + n].view(np.uint32)), want, f"sentinel, variant {variant}")
        f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, 0)
    f.close()


def test_degenerate_engines_and_odd_sizes(pkg):
    sp = QS.params(pkg)
    one = records(pkg, np.array([[0.2, -0.4, 0.1]], F), np.zeros((1, 3), F))
    f = pkg.SPHFluidGPU.from_particles(one, sp)
    x = np.array([[3.0, -2.0]], F)
    assert f.aggregate(x, 1.0).tolist() == [[0.0, 0.0]] and f.aggregate(x, 1.0, self_=True).tolist() == [[3.0, -2.0]]
    out, cnt = f.aggregate(x, 1.0, op="max", counts=True)
    assert np.isneginf(out).all() and cnt.tolist() == [0]
    assert f.query_aggregate(np.zeros((0, 3), F), x, 1.0).shape == (0, 2)                       # m = 0
    assert f.query_aggregate(np.array([[0.3, -0.4, 0.1]], F), x, 1.0, op="min").tolist() == [[3.0, -2.0]]
    with pytest.raises(pkg.SphError):
        f.aggregate(np.zeros((2, 2), F), 1.0)                                                    # two rows of values for one particle
    f.close()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    f = pkg.SPHFluidGPU.from_particles(none, sp)
    assert f.aggregate(np.zeros((0, 3), F), 1.0).shape == (0, 3)
    assert f.query_aggregate(np.zeros((5, 3), F), np.zeros((0, 3), F), 1.0, moments=True).shape == (5, 4, 3)
    f.close()
    for n in (257, 1023):                                                                        # no multiple of 64 or of the block
        rec, _ = QS.uniform(pkg, n, 40 + n)
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        for case in (PARTICLE_CASES[2], PARTICLE_CASES[7], PARTICLE_CASES[9]):
            _same(pkg, f, rec, sp, case, f"n {n}", variants=FEW)
        f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (1, 1, 0), (2, 1, 0), (3, 0, 0), (3, 1, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced: the rows are those of the downloaded records, and a later dispatch leaves a later call right."""
    def check(f, now, sp, what):
        for case in (PARTICLE_CASES[1], PARTICLE_CASES[2], PARTICLE_CASES[9]):
            _same(pkg, f, now, sp, case, what, variants=(0, 1))
        return None

    def unchanged(f, held):
        now = f.download()
        _same(pkg, f, now, f._p, PARTICLE_CASES[2], "after one more dispatch", variants=(0,))

    after_dispatches(pkg, kern, aos, graph, check, unchanged)


def test_aggregate_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()
    x = values_for(len(rec), 5)

    def probe(f):
        f.aggregate(x, 2.0 * sp.param_h, op="mean", weight="poly6", self_=True)
        f.aggregate(x, delta=True, moments=True)
        f.query_aggregate(pts, x, sp.param_h, op="max")

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def test_refusals(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    n, h = len(rec), sp.param_h
    x = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    pts = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    info = pkg.SphAggregateInfo()
    good = dict(radius=h, channels=4)

    def particles(e, cfg, values=x, out_=out, cnt_=cnt, info_=info):
        return L.sph_aggregate_particles(e, None if cfg is None else C.byref(cfg), None if values is None else vp(values.data_ptr()),
                                         None if out_ is None else vp(out_.data_ptr()), None if cnt_ is None else vp(cnt_.data_ptr()),
                                         None if info_ is None else C.byref(info_))

    def query(e, cfg, m=4):
        return L.sph_aggregate_query(e, C.byref(cfg), vp(pts.data_ptr()), m, vp(x.data_ptr()), vp(out.data_ptr()), vp(cnt.data_ptr()), C.byref(info))

    with slab_engine(pkg, rec, sp) as slab:
        assert particles(slab._h, pkg.aggregate_config(**good)) == -3 and b"slab" in L.sph_last_error()
        assert query(slab._h, pkg.aggregate_config(**good)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        assert particles(f._h, pkg.aggregate_config(**good)) == -3 and query(f._h, pkg.aggregate_config(**good)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.aggregate(x)
        with pytest.raises(pkg.SphError, match="-3"):
            f.query_aggregate(pts, x, h)
    assert particles(None, pkg.aggregate_config(**good)) == -1 and particles(f._h, None) == -1 and particles(f._h, pkg.aggregate_config(**good), info_=None) == -1
    assert particles(f._h, pkg.aggregate_config(**good), values=None) == -1 and particles(f._h, pkg.aggregate_config(**good), out_=None) == -1
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
        assert particles(f._h, pkg.aggregate_config(radius=R, channels=4)) == -1
    for bad in (dict(op=4), dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129),
                dict(op=pkg.SPH_AGGREGATE_MEAN, flags=pkg.SPH_AGGREGATE_MOMENTS), dict(op=pkg.SPH_AGGREGATE_MAX, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6)):
        assert particles(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
        assert query(f._h, pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):
        assert query(f._h, pkg.aggregate_config(flags=flag, **good)) == -1
    assert query(f._h, pkg.aggregate_config(**good), m=1 << 31) == -1
    flat = out.view(-1)
    assert particles(f._h, pkg.aggregate_config(**good), values=flat[8:], out_=flat) == -1 and b"overlap" in L.sph_last_error()
    assert particles(f._h, pkg.aggregate_config(**good), values=flat, out_=flat[n * 4 - 4:]) == -1
    assert particles(f._h, pkg.aggregate_config(**good), values=flat, out_=flat[n * 4:], cnt_=flat[n:]) == -1
    f.sync()
    assert (out == 7.0).all().item() and (cnt == 9).all().item()                                # no refused call wrote anything
    assert query(f._h, pkg.aggregate_config(**good), m=0) == 0 and (out == 7.0).all().item()
    # the option
    assert f.get_option(pkg.SPH_OPT_AGGREGATE_VARIANT) == 0
    for bad in (-1, 16):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_AGGREGATE_VARIANT, bad)
    assert particles(f._h, pkg.aggregate_config(**good)) == 0                                    # ... and the valid call works afterwards
    f.sync()
    assert (cnt.cpu().numpy().view(np.uint32) == np.diff(pkg.neighbors_host(rec, sp, h, count_only=True)[0])).all()
    f.close()


def test_velocity_differences_against_the_lists_and_index_add(pkg):
    """values = vel, delta: the fused SUM is the segmented fp32 sum in CSR order over neighbors(device=True), bit for bit, and README's
    index_add_ route (an order nobody fixes) within the float64 bound gamma_(count + 2) * sum |dv| (measured on this scene: at most
    0.51 of it; both routes add the same fp32 terms dv, so they differ by the rounding of the partial sums alone)."""
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(3)
    now = f.download()
    vel = torch.from_numpy(np.ascontiguousarray(now["vel"][:, :3])).cuda()
    out, cnt = f.aggregate(vel, delta=True, counts=True, device=True)
    off, idx = f.neighbors(device=True)
    assert torch.equal(cnt.to(torch.int64), off[1:] - off[:-1])
    recv = torch.repeat_interleave(torch.arange(len(rec), device="cuda"), off[1:] - off[:-1])
    dv = vel[idx.to(torch.int64)] - vel[recv]
    o, r, d = off.cpu().numpy(), recv.cpu().numpy(), dv.cpu().numpy()
    seq = np.zeros((len(rec), 3), F)
    rank = np.arange(len(r)) - o[r]
    for t in range(int(np.diff(o).max())):                                                      # sequential fp32 sums in CSR order
        e = np.flatnonzero(rank == t)
        seq[r[e]] = (seq[r[e]] + d[e]).astype(F)
    assert out.cpu().numpy().tobytes() == seq.tobytes()
    added = torch.zeros_like(vel).index_add_(0, recv, dv).cpu().numpy().astype(np.float64)
    mag = np.zeros((len(rec), 3))
    np.add.at(mag, r, np.abs(d.astype(np.float64)))
    bound = AR.gamma(np.diff(o).astype(np.float64) + 2)[:, None] * mag
    err = np.abs(out.cpu().numpy().astype(np.float64) - added)
    print(f"fused sum against index_add_: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    f.close()


def test_neighbor_mean_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "neighbor_mean", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "neighbor_mean OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
