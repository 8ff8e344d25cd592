"""Neighbour lists on the device (sph_neighbors.h) against sph_neighbors_host, bit for bit in offsets and indices, on the smallest
shapes where the kernels can go wrong; the interface around them; and the proof that building lists never changes the simulation."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import neighbors_ref as NR
import query_scenes as QS
from support import after_dispatches, build_example, linked_list_grid, records, run_example, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
FLAG_SETS = (dict(), dict(self_=True), dict(half=True), dict(count_only=True), dict(self_=True, count_only=True))


def _same(got, want, what):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), f"{what}: offsets differ"
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), f"{what}: indices differ"


def _check_engine(pkg, f, rec, sp, factors=(1.0, 2.0, 3.0), flag_sets=FLAG_SETS, what=""):
    """Every radius class (R exactly h, 2h, 3h by default) and every flag set: the device lists are the host lists."""
    for fac in factors:
        R = float(F(fac) * F(sp.param_h))
        for kw in flag_sets:
            want = pkg.neighbors_host(rec, sp, R, **kw)
            got = f.neighbors(R, **kw)
            _same(got, want, f"{what} R = {fac} h {kw}")
            if not kw.get("count_only"):                                          # the wave-cooperative fill: the same bits
                f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 1)
                _same(f.neighbors(R, **kw), want, f"{what} R = {fac} h {kw}, wave-cooperative fill")
                f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 0)
            info = f.neighbor_info()
            assert (info.rows, info.total, info.kind) == (len(rec), want[0][-1], 1) and info.radius == F(R)
            assert info.stencil == int(np.ceil(fac)) and info.maxCount == np.diff(want[0]).max()


def _check(pkg, rec, sp, **kw):
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    _check_engine(pkg, f, rec, sp, **kw)
    f.close()


@pytest.mark.parametrize("crowd", [63, 64, 65, 200, 300])
def test_crowded_cell(pkg, crowd):
    """A cell with more members than a wave (63 / 64 / 65) and than a block (300: its run of sorted slots crosses a block boundary),
    among a few hundred others: rows longer than a wave and than a block, targets of one block in many cells."""
    rec, sp, start, members = QS.crowded_cell(pkg, crowd)
    assert members >= crowd
    if crowd == 300:
        assert start // 256 != (start + members - 1) // 256, "the cell's run must cross a block boundary of sorted slots"
    _check(pkg, rec, sp, what=f"crowd {crowd}")


def test_edge_corner_and_clamped_cells(pkg):
    """Members of every corner and edge cell, and particles up to 30 % of the box beyond every face (clamped cells): the stencil is cut
    at the grid's faces and the relation stays symmetric."""
    rng = np.random.default_rng(2)
    sp = QS.params(pkg)
    lo, dims, cs = QS.grid(pkg, sp)
    corners = np.array([[x, y, z] for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)])
    corner_pos = lo + (np.repeat(corners, 6, axis=0).astype(F) + rng.random((48, 3)).astype(F)) * cs
    pos = np.concatenate([QS.grid_cloud(rng, (lo, dims, cs), 1500, beyond=0.3), corner_pos])
    rec = records(pkg, pos, np.zeros_like(pos))
    assert not NR.inside_grid(pkg, rec["pos"], sp)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    _check_engine(pkg, f, rec, sp, what="clamped")
    off, idx = f.neighbors(float(F(3.0) * F(sp.param_h)))
    fwd, back = NR.transpose_pairs(off, idx)
    assert np.array_equal(fwd, back) and len(idx)
    f.close()


def test_degenerate_engines(pkg):
    rng = np.random.default_rng(4)
    sp = QS.params(pkg)
    grid = QS.grid(pkg, sp)
    # one particle
    one = records(pkg, np.array([[0.2, -0.4, 0.1]], F), np.zeros((1, 3), F))
    _check(pkg, one, sp, what="n = 1")
    f = pkg.SPHFluidGPU.from_particles(one, sp)                                    # lists without a pair, as device tensors and as edges
    d_off, d_idx = f.neighbors(device=True)
    assert d_off.cpu().tolist() == [0, 0] and d_idx is not None and d_idx.numel() == 0
    assert tuple(f.radius_graph().shape) == (2, 0) and tuple(f.radius_graph(half=True).shape) == (2, 0)
    assert f.neighbors(count_only=True, device=True)[1] is None
    f.close()
    # ghosts and inactive records only: binned like any other record
    pos = QS.grid_cloud(rng, grid, 500)
    ghosts = records(pkg, pos, np.zeros_like(pos), ghost=np.where(np.arange(500) % 3 == 0, 3, 1).astype(np.int32))
    ghosts["isActive"] = np.arange(500) % 2
    _check(pkg, ghosts, sp, what="ghosts")
    assert pkg.neighbors_host(ghosts, sp, sp.param_h)[0][-1] > 0
    # non-finite positions: accepted by nobody, kept under SELF by identity
    bad = records(pkg, pos, np.zeros_like(pos))
    bad["pos"][7, 0] = np.nan
    bad["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(bad, sp)
    _check_engine(pkg, f, bad, sp, what="NaN")
    off, idx = f.neighbors(2.0 * sp.param_h)
    assert off[8] == off[7] and off[301] == off[300] and not np.isin(idx, (7, 300)).any()
    off, idx = f.neighbors(2.0 * sp.param_h, self_=True)
    assert idx[off[7]:off[8]].tolist() == [7] and idx[off[300]:off[301]].tolist() == [300]
    f.close()
    # a grid of 4 x 4 x 4 cells around a much larger box: s = 3 covers the whole grid from the middle cells, most particles are clamped
    small = QS.params(pkg, cap=4)
    assert list(pkg.compute_grid_extents(small).dims) == [4, 4, 4]
    pos = QS.grid_cloud(rng, grid, 700)
    _check(pkg, records(pkg, pos, np.zeros_like(pos)), small, what="grid_cap 4")


def test_radius_classes_between_the_cell_multiples(pkg):
    rng = np.random.default_rng(6)
    sp = QS.params(pkg)
    pos = QS.grid_cloud(rng, QS.grid(pkg, sp), 1200)
    rec = records(pkg, pos, np.zeros_like(pos))
    up = float(np.nextafter(F(sp.param_h), F(np.inf))) / sp.param_h              # the first radius of class s = 2
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac, s in ((0.5, 1), (up, 2), (1.5, 2), (2.5, 3)):
        R = float(F(fac) * F(sp.param_h))
        _same(f.neighbors(R), pkg.neighbors_host(rec, sp, R), f"R = {fac} h")
        assert f.neighbor_info().stencil == s
    assert f.neighbors()[0][-1] == pkg.neighbors_host(rec, sp, sp.param_h)[0][-1]   # radius None: param_h
    f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (2, 1, 0), (1, 1, 0), (3, 0, 0), (3, 1, 1), (3, 0, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced (every SPH pass variant, lazy and eager records, a replayed graph): the lists are those of the
    downloaded records, and at R = h with SELF the degrees are the sampler's counts."""
    def check(f, now, sp, what):
        _check_engine(pkg, f, now, sp, factors=(1.0, 2.0), flag_sets=(dict(), dict(half=True)), what=what)
        off, idx = f.neighbors(self_=True)
        assert np.array_equal(np.diff(off), f.sample(now["pos"][:, :3])["count"].astype(np.int64))
        return off, idx

    def unchanged(f, held):                                                        # the lists describe the state they were built from
        _same(f.neighbor_lists(), held, "after a dispatch")

    after_dispatches(pkg, kern, aos, graph, check, unchanged)


def test_query_lists(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg, 700)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac in (1.0, 2.0, 3.0):
        R = float(F(fac) * F(sp.param_h))
        want = pkg.neighbors_host(rec, sp, R, points=pts)
        _same(f.query_neighbors(pts, R), want, f"query R = {fac} h")
        f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 1)
        _same(f.query_neighbors(pts, R), want, f"query R = {fac} h, wave-cooperative fill")
        f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 0)
        info = f.neighbor_info()
        assert (info.rows, info.total, info.kind, info.stencil) == (700, want[0][-1], 2, int(fac))
        assert want[0][6] == want[0][5] and want[0][257] == want[0][256] and want[0][700] == want[0][699] and want[0][-1] > 0
        _same(f.query_neighbors(pts, R, count_only=True), (want[0], None), "query, count only")
    # the particles' own positions as queries: the SELF rows; a device tensor is used in place
    R = sp.param_h
    p4 = torch.from_numpy(np.ascontiguousarray(rec["pos"])).cuda()
    _same(f.query_neighbors(p4, R), pkg.neighbors_host(rec, sp, R, self_=True), "positions as queries")
    f.close()


def test_device_tensors_and_radius_graph(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(2)
    off, idx = f.neighbors(1.5 * sp.param_h)
    d_off, d_idx = f.neighbors(1.5 * sp.param_h, device=True)
    assert d_off.is_cuda and d_off.dtype == torch.int64 and d_idx.is_cuda and d_idx.dtype == torch.int32
    assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_idx.cpu().numpy(), idx)
    c_off, c_idx = f.neighbors(1.5 * sp.param_h, count_only=True, device=True)
    assert c_idx is None and np.array_equal(c_off.cpu().numpy(), off)
    # borrowed addresses
    a, b = vp(), vp()
    f.neighbors(1.5 * sp.param_h)
    assert pkg.load_library().sph_neighbors_device(f._h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    # edges
    g = f.radius_graph(1.5 * sp.param_h)
    assert g.shape == (2, len(idx)) and g.dtype == torch.int64 and g.is_cuda
    assert np.array_equal(torch.bincount(g[0], minlength=len(rec)).cpu().numpy(), np.diff(off))
    assert np.array_equal(g[1].cpu().numpy(), idx.astype(np.int64))
    gh = f.radius_graph(1.5 * sp.param_h, half=True)
    assert gh.shape[1] * 2 == g.shape[1] and bool((gh[0] < gh[1]).all())
    # a per-particle sum over the edges: the degree again
    deg = torch.zeros(len(rec), device="cuda").index_add_(0, g[0], torch.ones(g.shape[1], device="cuda"))
    assert np.array_equal(deg.cpu().numpy().astype(np.int64), np.diff(off))
    f.close()


def test_max_pairs_refusal_leaves_valid_offsets(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = pkg.neighbors_host(rec, sp, sp.param_h)
    total = int(want[0][-1])
    with pytest.raises(pkg.SphError, match="-4"):
        f.neighbors(max_pairs=total - 1)
    info = f.neighbor_info()
    assert (info.rows, info.total, info.kind) == (len(rec), total, 1)
    _same(f.neighbor_lists(), (want[0], None), "after the refusal")
    d_off, d_idx = f.neighbor_lists(device=True)
    assert d_idx is None and np.array_equal(d_off.cpu().numpy(), want[0])
    _same(f.neighbors(max_pairs=total), want, "max_pairs == total")
    f.close()


def test_export_download_states_and_arguments(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    n = len(rec)
    off = np.zeros(n + 1, np.int64)
    big = np.zeros(1 << 20, np.int32)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_big = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")
    a, b = vp(), vp()

    def nothing_held():
        assert L.sph_neighbors_download(f._h, off.ctypes.data_as(vp), big.ctypes.data_as(vp), len(big)) == -3
        assert L.sph_neighbors_export(f._h, vp(d_off.data_ptr()), vp(d_big.data_ptr()), len(big)) == -3
        assert L.sph_neighbors_device(f._h, C.byref(a), C.byref(b)) == -3
        assert f.neighbor_info().kind == 0
    nothing_held()                                                                 # before any build
    want = pkg.neighbors_host(rec, sp, sp.param_h)
    total = int(want[0][-1])
    _same(f.neighbors(), want, "build")
    # a short cap: nothing written
    assert L.sph_neighbors_download(f._h, off.ctypes.data_as(vp), big.ctypes.data_as(vp), total - 1) == -4
    assert L.sph_neighbors_export(f._h, vp(d_off.data_ptr()), vp(d_big.data_ptr()), total - 1) == -4
    f.sync()
    assert not off.any() and not big.any() and not bool(d_off.any()) and not bool(d_big.any())
    # null arguments
    assert L.sph_neighbors_download(f._h, None, big.ctypes.data_as(vp), len(big)) == -1
    assert L.sph_neighbors_download(f._h, off.ctypes.data_as(vp), None, len(big)) == -1
    assert L.sph_neighbors_export(None, vp(d_off.data_ptr()), vp(d_big.data_ptr()), len(big)) == -1
    assert L.sph_neighbors_device(f._h, None, C.byref(b)) == -1
    info = pkg.SphNeighborInfo()
    assert L.sph_neighbors_build(f._h, sp.param_h, 0, 0, None) == -1 and L.sph_neighbors_info(f._h, None) == -1
    assert L.sph_neighbors_query(f._h, None, 4, sp.param_h, 0, 0, C.byref(info)) == -1
    assert L.sph_neighbors_query(f._h, vp(d_big.data_ptr()), 0, sp.param_h, 0, 0, C.byref(info)) == -1
    # arguments of the radius and the flags
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * sp.param_h):
        assert L.sph_neighbors_build(f._h, R, 0, 0, C.byref(info)) == -1
    assert L.sph_neighbors_build(f._h, sp.param_h, 3, 0, C.byref(info)) == -1       # SELF | HALF
    assert L.sph_neighbors_build(f._h, sp.param_h, 8, 0, C.byref(info)) == -1
    for fl in (1, 2):
        assert L.sph_neighbors_query(f._h, vp(d_big.data_ptr()), 4, sp.param_h, fl, 0, C.byref(info)) == -1
    _same(f.neighbor_lists(), want, "refused calls leave the lists alone")
    assert f.get_option(pkg.SPH_OPT_NEIGHBORS_FILL) == 0
    for bad in (-1, 2):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, bad)
    f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 1)
    assert f.get_option(pkg.SPH_OPT_NEIGHBORS_FILL) == 1
    f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 0)
    # an exact cap is enough
    assert L.sph_neighbors_download(f._h, off.ctypes.data_as(vp), big.ctypes.data_as(vp), total) == 0
    assert np.array_equal(off, want[0]) and np.array_equal(big[:total], want[1]) and not big[total:].any()
    # sph_reset ends the lists
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_refused_on_slab_engines_and_linked_list_grid(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    info = pkg.SphNeighborInfo()
    pts = torch.zeros(16, dtype=torch.float32, device="cuda")
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_neighbors_build(slab._h, sp.param_h, 0, 0, C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_neighbors_query(slab._h, vp(pts.data_ptr()), 4, sp.param_h, 0, 0, C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.neighbors()
        with pytest.raises(pkg.SphError, match="-3"):
            f.query_neighbors(rec["pos"][:4, :3], sp.param_h)
        assert f.neighbor_info().kind == 0
    _same(f.neighbors(), pkg.neighbors_host(rec, sp, sp.param_h), "grid build 0 again")
    f.close()


def test_lists_do_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()

    def probe(f):
        f.neighbors(2.0 * sp.param_h, half=True)
        f.query_neighbors(pts, sp.param_h)

    for aos in (1, 0):
        for graph in (0, 1):
            a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
            b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
            assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
            assert_records_equal(a, b, f"aos {aos} graph {graph}")
            if graph:
                assert la > 0 and lb > 0


def test_neighbor_lists_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "neighbor_lists", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "neighbor_lists OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
