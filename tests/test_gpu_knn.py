"""k nearest neighbours on the device (sph_knn.h) against sph_knn_host, byte for byte in indices, dist2 (as uint32 bits), counts and info,
for the default kernel (LDS rows) AND the selection kernel (SPH_OPT_KNN_VARIANT 1), on the smallest shapes where they can go wrong; the
interface around them; and the proof that a build changes neither the simulation nor the other query results."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import neighbors_ref as NR
import query_scenes as QS
from support import after_dispatches, build_example, linked_list_grid, records, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
INFO_FIELDS = ("rows", "total", "rowsFull", "radius", "k", "stencil", "flags", "kind")


def _equal(got, want, what):
    (idx, d2, cnt), (w_idx, w_d2, w_cnt) = got, want[:3]
    assert idx.dtype == np.int32 and d2.dtype == F and cnt.dtype == np.uint32, what
    assert idx.shape == w_idx.shape and d2.shape == w_d2.shape and cnt.shape == w_cnt.shape, what
    assert cnt.tobytes() == w_cnt.tobytes(), f"{what}: counts differ"
    assert idx.tobytes() == w_idx.tobytes(), f"{what}: indices differ"
    assert d2.view(np.uint32).tobytes() == w_d2.view(np.uint32).tobytes(), f"{what}: dist2 bits differ"


def _same(pkg, f, rec, sp, k, R, points=None, dev_points=None, what="", **kw):
    """Both variants give sph_knn_host's bytes and info; returns the host result."""
    want = pkg.knn_host(rec, sp, k, R, points=points, **kw)
    for variant in (0, 1):
        f.set_option(pkg.SPH_OPT_KNN_VARIANT, variant)
        if points is None:
            got = f.knn(k, R, **kw)
        else:
            got = f.query_knn(points if dev_points is None else dev_points, k, R, **kw)
        _equal(got, want, f"{what} k {k} R {R} {kw} variant {variant}")
        same_info(f.knn_info(), want[3], INFO_FIELDS, f"{what} k {k} R {R} variant {variant}")
    f.set_option(pkg.SPH_OPT_KNN_VARIANT, 0)
    return want


def _h(sp, fac):
    return float(F(fac) * F(sp.param_h))


@pytest.mark.parametrize("crowd", [63, 64, 65, 300])
def test_crowded_cell(pkg, crowd):
    """A cell with 63 / 64 / 65 / 300 members among 400 others: far more accepted candidates than any row keeps, in one run of sorted
    slots (300: a run that crosses a block boundary of every class), so a full row is overwritten many times."""
    rec, sp, start, members = QS.crowded_cell(pkg, crowd)
    assert members >= crowd
    if crowd == 300:
        assert start // 256 != (start + members - 1) // 256, "the cell's run must cross a block boundary of sorted slots"
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    deg = np.diff(pkg.neighbors_host(rec, sp, _h(sp, 2.0))[0])
    assert deg[400:].min() >= crowd - 1                                           # every member of the cell sees all the others within 2h
    for k in (8, 16, 64):
        _same(pkg, f, rec, sp, k, _h(sp, 1.0), what=f"crowd {crowd}")
        want = _same(pkg, f, rec, sp, k, _h(sp, 2.0), self_=True, what=f"crowd {crowd}")
        assert (want[2][400:] == min(k, crowd)).all() or crowd < k
    f.close()


@pytest.mark.parametrize("fac", [1.0, 2.0, 3.0, 1.3])
def test_every_class_edge_and_radius_class(pkg, fac):
    rec, sp = QS.uniform(pkg, 1200, seed=31)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    R = _h(sp, fac)
    res = {}
    for k in (1, 8, 9, 16, 17, 32, 33, 64):
        res[k] = _same(pkg, f, rec, sp, k, R, what=f"R = {fac} h")
        assert res[k][3].stencil == int(np.ceil(fac))
    # the row for k1 is a prefix of the row for k2 > k1; counts are min(k, degree) of the neighbour lists at the same R
    deg = np.diff(f.neighbors(R, count_only=True)[0])
    i64, d64, c64, _ = res[64]
    for k, (idx, d2, cnt, _) in res.items():
        keep = np.arange(k)[None, :] < cnt[:, None]
        assert np.array_equal(cnt, np.minimum(deg, k)) and np.array_equal(idx[keep], i64[:, :k][keep])
        assert np.array_equal(d2.view(np.uint32)[keep], d64.view(np.uint32)[:, :k][keep])
    # k >= the degree: the neighbour list's ids, in another order
    off, nidx = f.neighbors(R)
    for i in np.flatnonzero(deg <= 64)[:200]:
        assert np.array_equal(np.sort(i64[i, :c64[i]]), np.sort(nidx[off[i]:off[i + 1]]))
    assert f.knn(8)[0].tobytes() == pkg.knn_host(rec, sp, 8, sp.param_h)[0].tobytes()           # radius None: param_h
    f.close()


def test_edge_corner_and_clamped_cells(pkg):
    """Members of every corner cell and particles up to 30 % of the box beyond every face (clamped cells): the stencil is cut at the
    grid's faces, and far-away particles share a clamped cell."""
    rng = np.random.default_rng(2)
    sp = QS.params(pkg)
    lo, dims, cs = QS.grid(pkg, sp)
    corners = np.array([[x, y, z] for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)])
    corner_pos = lo + (np.repeat(corners, 6, axis=0).astype(F) + rng.random((48, 3)).astype(F)) * cs
    pos = np.concatenate([QS.grid_cloud(rng, (lo, dims, cs), 1500, beyond=0.3), corner_pos])
    rec = records(pkg, pos, np.zeros_like(pos))
    assert not NR.inside_grid(pkg, rec["pos"], sp)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for k, fac in ((8, 1.0), (16, 2.0), (33, 3.0), (64, 3.0)):
        _same(pkg, f, rec, sp, k, _h(sp, fac), what="clamped")
    _same(pkg, f, rec, sp, 16, _h(sp, 2.0), self_=True, what="clamped")
    # a grid of 4 x 4 x 4 cells around a much larger box: s = 3 covers the whole grid from the middle cells, most particles are clamped
    small = QS.params(pkg, cap=4)
    assert list(pkg.compute_grid_extents(small).dims) == [4, 4, 4]
    pos = QS.grid_cloud(rng, (lo, dims, cs), 700)
    rec = records(pkg, pos, np.zeros_like(pos))
    g = pkg.SPHFluidGPU.from_particles(rec, small)
    for k, fac in ((8, 1.0), (64, 3.0)):
        _same(pkg, g, rec, small, k, _h(small, fac), what="grid_cap 4")
    g.close()
    f.close()


def test_tie_order_on_the_device(pkg):
    """The exact lattice (whole shells tie) and eight coincident particles (runs of r2 = 0): ties resolve by id on the device too."""
    rec, sp = QS.lattice(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for k, R in ((6, 0.5), (7, 0.5), (19, 1.0), (64, 1.0)):
        idx, d2, cnt, _ = _same(pkg, f, rec, sp, k, R, what="lattice")
        tied = (d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])
        assert tied.any() and (idx[:, 1:][tied] > idx[:, :-1][tied]).all()
    f.close()
    rec, sp, same = QS.coincident(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for k in (4, 8, 16):
        idx, d2, _, _ = _same(pkg, f, rec, sp, k, 1.0, self_=True, what="coincident")
        assert all(idx[i, :min(k, 8)].tolist() == same[:min(k, 8)].tolist() for i in same)
        idx, d2, _, _ = _same(pkg, f, rec, sp, k, 1.0, what="coincident")
        assert all(idx[i, :min(k, 7)].tolist() == same[same != i][:min(k, 7)].tolist() for i in same)
    f.close()


def test_short_rows_ghosts_and_non_finite_particles(pkg):
    # a sparse background: most rows shorter than k, padded; k > n
    rec, sp = QS.uniform(pkg, 150, seed=32)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for k, fac in ((8, 1.0), (16, 2.0), (64, 3.0)):
        idx, d2, cnt, info = _same(pkg, f, rec, sp, k, _h(sp, fac), what="sparse")
        assert (cnt < k).any() and (idx[np.arange(k)[None, :] >= cnt[:, None]] == -1).all()
    f.close()
    rec, sp = QS.uniform(pkg, 20, seed=25)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, 64, 1.5, what="k > n")
    assert want[3].rowsFull == 0 and want[3].total > 0
    f.close()
    # ghosts of every kind, inactive records: candidates like any other, unless FLUID_ONLY
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for kw in (dict(), dict(fluid_only=True), dict(fluid_only=True, self_=True)):
        for k, fac in ((8, 2.0), (33, 3.0)):
            idx, d2, cnt, _ = _same(pkg, f, rec, sp, k, _h(sp, fac), what="ghosts", **kw)
            if kw:
                assert (cnt[ghost] == 0).all() and not ghost[idx[idx >= 0]].any() and (cnt[~ghost] > 0).all()
    _same(pkg, f, rec, sp, 8, 1.0, points=rec["pos"][:333, :3], fluid_only=True, what="ghosts, query")
    f.close()
    # non-finite positions: accepted by nobody, an empty row also under SELF
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for self_ in (False, True):
        idx, d2, cnt, _ = _same(pkg, f, rec, sp, 16, 1.0, self_=self_, what="NaN")
        assert cnt[7] == 0 and cnt[300] == 0 and not np.isin(idx, (7, 300)).any()
    f.close()


def test_degenerate_engines(pkg):
    sp = QS.params(pkg)
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    f = pkg.SPHFluidGPU.from_particles(none, sp)
    want = _same(pkg, f, none, sp, 8, 1.0, what="n = 0")
    assert want[0].shape == (0, 8) and f.knn_info().kind == 1
    pts = np.zeros((5, 3), F)
    idx, d2, cnt, _ = _same(pkg, f, none, sp, 8, 1.0, points=pts, what="n = 0, query")
    assert (idx == -1).all() and cnt.tolist() == [0] * 5
    f.close()
    one = records(pkg, np.array([[0.2, -0.4, 0.1]], F), np.zeros((1, 3), F))
    f = pkg.SPHFluidGPU.from_particles(one, sp)
    assert _same(pkg, f, one, sp, 4, 1.0, what="n = 1")[0].tolist() == [[-1] * 4]
    assert _same(pkg, f, one, sp, 4, 1.0, self_=True, what="n = 1")[0].tolist() == [[0, -1, -1, -1]]
    want = _same(pkg, f, one, sp, 4, 1.0, points=np.zeros((0, 3), F), what="m = 0")
    assert want[0].shape == (0, 4) and f.knn_info().kind == 2 and f.knn_info().rows == 0
    assert tuple(f.knn_graph(4).shape) == (2, 0)
    f.close()
    # all particles in one cell
    rng = np.random.default_rng(33)
    lo, dims, cs = QS.grid(pkg, sp)
    pos = lo + (np.array([4, 3, 3], F) + F(0.02) + F(0.96) * rng.random((300, 3)).astype(F)) * cs
    rec = records(pkg, pos, np.zeros_like(pos))
    assert len(np.unique(NR.cells(pkg, rec["pos"], sp))) == 1
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, 64, 1.0, what="one cell")
    assert want[3].rowsFull == 300
    f.close()


def test_query_rows(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for k, fac in ((8, 1.0), (17, 2.0), (64, 3.0)):
        idx, d2, cnt, info = _same(pkg, f, rec, sp, k, _h(sp, fac), points=pts, what="query")
        assert cnt[5] == 0 and cnt[256] == 0 and cnt[700] == 0 and info.total > 0 and info.kind == 2
    # a torch device tensor of (m, 4) is used in place; the particles' own positions as queries are the SELF rows
    p4 = torch.from_numpy(np.ascontiguousarray(rec["pos"])).cuda()
    q = _same(pkg, f, rec, sp, 16, 1.0, points=rec["pos"][:, :3], dev_points=p4, what="positions as queries")
    s = pkg.knn_host(rec, sp, 16, 1.0, self_=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(q[:3], s[:3]))
    f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (1, 1, 0), (3, 0, 0), (3, 1, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced: the rows are those of the downloaded records, and a later dispatch does not touch them."""
    def check(f, now, sp, what):
        _same(pkg, f, now, sp, 8, _h(sp, 1.0), what=what)
        return _same(pkg, f, now, sp, 33, _h(sp, 2.0), what=what)

    def unchanged(f, want):
        _equal(f.knn_rows(), want, "after a dispatch")

    after_dispatches(pkg, kern, aos, graph, check, unchanged)


def test_device_tensors_and_knn_graph(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(2)
    now = f.download()
    R = _h(sp, 1.5)
    w_idx, w_d2, w_cnt, w_info = pkg.knn_host(now, sp, 12, R)
    idx, d2, cnt = f.knn(12, R, device=True)
    assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == (len(rec), 12) == tuple(d2.shape)
    assert np.array_equal(idx.cpu().numpy(), w_idx) and np.array_equal(cnt.cpu().numpy().astype(np.uint32), w_cnt)
    assert d2.cpu().numpy().view(np.uint32).tobytes() == w_d2.view(np.uint32).tobytes()
    a, b, c = vp(), vp(), vp()
    assert pkg.load_library().sph_knn_device(f._h, C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value and b.value and c.value
    # edges: the host rows expanded in row order, then rank order
    g = f.knn_graph(12, R)
    keep = w_idx >= 0
    recv = np.broadcast_to(np.arange(len(rec))[:, None], w_idx.shape)[keep]
    assert g.is_cuda and g.dtype == torch.int64 and tuple(g.shape) == (2, int(w_info.total)) and g.shape[1] == f.knn_info().total
    assert np.array_equal(g[0].cpu().numpy(), recv) and np.array_equal(g[1].cpu().numpy(), w_idx[keep].astype(np.int64))
    gs = f.knn_graph(12, R, self_=True)
    s_idx = pkg.knn_host(now, sp, 12, R, self_=True)[0]
    assert np.array_equal(gs[1].cpu().numpy(), s_idx[s_idx >= 0].astype(np.int64)) and gs.shape[1] == f.knn_info().total
    dq = f.query_knn(now["pos"][:100, :3], 5, R, device=True)
    assert tuple(dq[0].shape) == (100, 5) and np.array_equal(dq[0].cpu().numpy(), pkg.knn_host(now, sp, 5, R, points=now["pos"][:100, :3])[0])
    f.close()


def test_coexists_with_neighbour_lists_and_components(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    R = _h(sp, 1.5)
    lists = f.neighbors(R)
    rows = f.knn(16, R)
    comp = f.components(0.6 * sp.param_h)
    again = f.neighbor_lists()
    assert np.array_equal(again[0], lists[0]) and np.array_equal(again[1], lists[1])
    _equal(f.knn_rows(), rows, "after components()")
    _equal(rows, pkg.knn_host(rec, sp, 16, R), "knn between neighbors() and components()")
    want = pkg.neighbors_host(rec, sp, R)
    assert np.array_equal(lists[0], want[0]) and np.array_equal(lists[1], want[1])
    assert comp[0].tobytes() == pkg.components_host(rec, sp, 0.6 * sp.param_h)[0].tobytes()
    f.neighbors(_h(sp, 1.0))                                                       # ... and the other way round
    _equal(f.knn_rows(), rows, "after neighbors()")
    f.close()


def test_knn_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()

    def probe(f):
        f.knn(16, 2.0 * sp.param_h)
        f.query_knn(pts, 8, sp.param_h)

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def test_refusals_and_states(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    info = pkg.SphKnnInfo()
    pts = torch.zeros(16, dtype=torch.float32, device="cuda")
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_knn_build(slab._h, 8, sp.param_h, 0, C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_knn_query(slab._h, vp(pts.data_ptr()), 4, 8, sp.param_h, 0, C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    n = len(rec)
    idx, d2, cnt = np.full((n, 8), 9, np.int32), np.zeros((n, 8), F), np.zeros(n, np.uint32)
    a, b, c = vp(), vp(), vp()

    def nothing_held():
        assert L.sph_knn_info(f._h, C.byref(info)) == -3
        assert L.sph_knn_device(f._h, C.byref(a), C.byref(b), C.byref(c)) == -3
        assert L.sph_knn_download(f._h, idx.ctypes.data_as(vp), d2.ctypes.data_as(vp), cnt.ctypes.data_as(vp)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.knn_info()
        assert (idx == 9).all()
    nothing_held()                                                                 # before any build
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.knn(8)
        with pytest.raises(pkg.SphError, match="-3"):
            f.query_knn(rec["pos"][:4, :3], 8, sp.param_h)
    nothing_held()
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * sp.param_h):
        assert L.sph_knn_build(f._h, 8, R, 0, C.byref(info)) == -1
    for k in (0, -1, 65):
        assert L.sph_knn_build(f._h, k, sp.param_h, 0, C.byref(info)) == -1
        assert L.sph_knn_query(f._h, vp(pts.data_ptr()), 4, k, sp.param_h, 0, C.byref(info)) == -1
    assert L.sph_knn_build(f._h, 8, sp.param_h, 4, C.byref(info)) == -1            # an unknown flag bit
    assert L.sph_knn_query(f._h, vp(pts.data_ptr()), 4, 8, sp.param_h, pkg.SPH_KNN_SELF, C.byref(info)) == -1
    assert L.sph_knn_build(f._h, 8, sp.param_h, 0, None) == -1 and L.sph_knn_build(None, 8, sp.param_h, 0, C.byref(info)) == -1
    assert L.sph_knn_query(f._h, None, 4, 8, sp.param_h, 0, C.byref(info)) == -1
    assert L.sph_knn_query(f._h, vp(pts.data_ptr()), 1 << 31, 8, sp.param_h, 0, C.byref(info)) == -1
    nothing_held()
    want = pkg.knn_host(rec, sp, 8, sp.param_h)
    _equal(f.knn(8), want, "build")
    assert L.sph_knn_build(f._h, 65, sp.param_h, 0, C.byref(info)) == -1           # a refused call leaves the rows alone
    _equal(f.knn_rows(), want, "after a refused call")
    assert L.sph_knn_device(f._h, None, C.byref(b), C.byref(c)) == -1 and L.sph_knn_info(f._h, None) == -1
    # null pointers are skipped by the download; device memory is told from host memory by the address
    assert L.sph_knn_download(f._h, None, None, cnt.ctypes.data_as(vp)) == 0 and np.array_equal(cnt, want[2]) and (idx == 9).all()
    d_idx = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                                       # (the fill runs on torch's stream, the copy on the engine's own)
    assert L.sph_knn_download(f._h, vp(d_idx.data_ptr()), d2.ctypes.data_as(vp), None) == 0
    assert np.array_equal(d_idx.cpu().numpy(), want[0]) and d2.view(np.uint32).tobytes() == want[1].view(np.uint32).tobytes()
    # the option
    assert f.get_option(pkg.SPH_OPT_KNN_VARIANT) == 0
    for bad in (-1, 2):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_KNN_VARIANT, bad)
    # valid after a dispatch, ended by a reset
    f.DispatchN(2)
    assert f.knn_info().total == want[3].total
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_knn_spacing_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "knn_spacing", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "knn_spacing OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
