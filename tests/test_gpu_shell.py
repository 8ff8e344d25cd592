"""Free-surface particles on the device (sph_shell.h) against sph_shell_host, byte for byte in the 32-byte rows (crest included), ids
and info, on the smallest shapes where the kernels can go wrong; the interface around them; and the proof that a build changes
neither the simulation nor the other query results."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME, assert_records_equal, small_scene
import neighbors_ref as NR
import query_scenes as QS
import rays_scenes as RS
import shell_scenes as SS
from support import after_dispatches, build_example, linked_list_grid, records, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
INFO_FIELDS = ("rows", "numShell", "numIsolated", "maxCount", "radius", "stencil", "kind", "flags")


def _scan_tile():
    """kScanTile of csrc/sph_kernels.h: 256 threads times SPH_SCAN_ITEMS."""
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "sph_kernels.h")).read()
    return 256 * int(re.search(r"#define SPH_SCAN_ITEMS (\d+)", src).group(1))


def _equal(got, want, what):
    (rows, ids), (w_rows, w_ids) = got[:2], want[:2]
    assert rows.dtype == w_rows.dtype and rows.shape == w_rows.shape and ids.dtype == np.int32, what
    if rows.tobytes() != w_rows.tobytes():
        for key in rows.dtype.names:
            bad = np.flatnonzero((np.ascontiguousarray(rows[key]).view(np.uint32).reshape(len(rows), -1) !=
                                  np.ascontiguousarray(w_rows[key]).view(np.uint32).reshape(len(rows), -1)).any(axis=1))
            assert not len(bad), f"{what}: {key} differs on {len(bad)} of {len(rows)} rows, first {bad[:5].tolist()}: {rows[key][bad[:3]].tolist()} against {w_rows[key][bad[:3]].tolist()}"
    assert np.array_equal(ids, w_ids), f"{what}: ids differ"


def _same(pkg, f, rec, sp, R=None, points=None, dev_points=None, what="", **kw):
    """The device gives sph_shell_host's bytes and info; returns the host result."""
    want = pkg.shell_host(rec, sp, R, points=points, **kw)
    if points is None:
        got = f.shell(R, **kw)
    else:
        got = f.query_shell(points if dev_points is None else dev_points, R, **kw)
    _equal(got, want, f"{what} R {R} {kw}")
    same_info(f.shell_info(), want[2], INFO_FIELDS, f"{what} R {R} {kw}")
    return want


def _h(sp, fac):
    return float(F(fac) * F(sp.param_h))


@pytest.mark.parametrize("fac", [1.0, 1.3, 2.0, 3.0])
def test_edges_of_the_grid(pkg, fac):
    """The uniform box and a cloud up to a quarter of the grid's extent beyond every face (edge, corner and clamped cells), at every
    radius class."""
    rec, sp = QS.uniform(pkg, 3000, seed=31)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, _h(sp, fac), what="uniform")
    assert want[2].stencil == int(np.ceil(fac)) and 0 < want[2].numShell < len(rec) and (want[0]["crest"] > 0).any()
    f.close()
    rng = np.random.default_rng(2)
    grid = QS.grid(pkg, sp)
    lo, dims, cs = grid
    corners = np.array([[x, y, z] for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)])
    corner_pos = lo + (np.repeat(corners, 6, axis=0).astype(F) + rng.random((48, 3)).astype(F)) * cs
    pos = np.concatenate([QS.grid_cloud(rng, grid, 2500, beyond=0.25), corner_pos])
    rec = records(pkg, pos, np.zeros_like(pos))
    assert not NR.inside_grid(pkg, rec["pos"], sp)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    _same(pkg, f, rec, sp, _h(sp, fac), what="clamped")
    f.close()


def test_crowded_cell(pkg):
    """One cell of 300 members among 400 others: long runs of one lane, a run of sorted slots that crosses a block boundary."""
    rec, sp, _, _ = QS.crowded_cell(pkg, 300)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac in (1.0, 2.0):
        want = _same(pkg, f, rec, sp, _h(sp, fac), what="crowd")
        assert want[2].maxCount >= (299 if fac == 2.0 else 100)                    # (within 2h every member of the cell sees all the others)
    _same(pkg, f, rec, sp, _h(sp, 1.0), offset=0.0, what="crowd, all shell")       # pass 2 over every member of the cell
    f.close()


def test_special_records(pkg):
    rec, sp = QS.with_ghosts(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for kw in (dict(), dict(fluid_only=True)):
        for fac in (2.0, 3.0):
            want = _same(pkg, f, rec, sp, _h(sp, fac), what="ghosts", **kw)
            if kw:
                ghost = rec["isGhost"] != 0
                assert (want[0][ghost].view(np.uint8) == 0).all() and not np.isin(want[1], np.flatnonzero(ghost)).any()
    _same(pkg, f, rec, sp, 1.0, points=rec["pos"][:333, :3], fluid_only=True, what="ghosts, query")
    f.close()
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, 1.0, what="non-finite")
    assert (want[0][[7, 300]].view(np.uint8) == 0).all()
    f.close()
    rec, sp, same = QS.coincident(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, 1.0, what="coincident")
    assert len({want[0][i].tobytes() for i in same}) == 1
    _same(pkg, f, rec, sp, 1.0, offset=0.0, what="coincident, all shell")
    f.close()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_tiny_engines(pkg, n):
    sp = QS.params(pkg)
    rec = QS.uniform(pkg, max(n, 1), seed=5)[0][:n]
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    want = _same(pkg, f, rec, sp, 1.0, what=f"n = {n}")
    assert want[2].kind == 1 and want[2].rows == n
    if n == 1:
        assert want[0]["flags"].tolist() == [3] and want[1].tolist() == [0]
    _same(pkg, f, rec, sp, 1.0, offset=0.0, min_count=2 ** 32 - 1, what=f"n = {n}, all shell")
    q = _same(pkg, f, rec, sp, 1.0, points=np.zeros((5, 3), F), what=f"n = {n}, query")
    assert q[2].kind == 2 and (q[0]["crest"] == 0).all()
    q = _same(pkg, f, rec, sp, 1.0, points=np.zeros((0, 3), F), what=f"n = {n}, m = 0")
    assert q[2].rows == 0 and f.shell_info().kind == 2
    f.close()


def test_scan_tile_seams(pkg):
    """Particle counts around the scan's tile (kScanTile - 1, kScanTile, kScanTile + 1, 2 kScanTile + 1): the compactions of ids and of
    the shell slots cross tile seams; a scene with no shell at all (the threshold out of reach) and one that is all shell."""
    tile = _scan_tile()
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        rec, sp = QS.uniform(pkg, n, seed=n)
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        want = _same(pkg, f, rec, sp, 1.0, what=f"n = {n}")
        assert 0 < want[2].numShell < n
        none = _same(pkg, f, rec, sp, 1.0, offset=1e30, min_count=0, what=f"n = {n}, no shell")
        assert none[2].numShell == none[2].numIsolated and len(none[1]) == none[2].numShell and (none[0]["crest"] == 0).all()
        every = _same(pkg, f, rec, sp, 1.0, offset=0.0, min_count=2 ** 32 - 1, what=f"n = {n}, all shell")
        assert every[2].numShell == n and np.array_equal(every[1], np.arange(n, dtype=np.int32))
        f.close()


def test_ball_crest(pkg):
    """The ball of radius 5 dx: pass 2 on the device against the twin, crest bytes included, at R = h and R = 2h."""
    rec, sp, _ = SS.ball(pkg, 5.0)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac in (1.0, 2.0):
        want = _same(pkg, f, rec, sp, _h(sp, fac), what="ball")
        member = (want[0]["flags"] & 1) != 0
        assert member.sum() > 100 and (want[0]["crest"][member] > 0).mean() > 0.9
    f.close()


def test_query_rows(pkg):
    import torch
    rec, sp, pts = QS.query_cloud(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac in (1.0, 2.0, 3.0):
        rows, ids, info = _same(pkg, f, rec, sp, _h(sp, fac), points=pts, what="query")
        assert (rows[[5, 256, 700]].view(np.uint8) == 0).all() and info.kind == 2 and (rows["crest"] == 0).all() and info.numShell > 0
    # a torch device tensor of (m, 4) is used in place; a particle's own position as a query counts the particle itself
    p4 = torch.from_numpy(np.ascontiguousarray(rec["pos"])).cuda()
    q = _same(pkg, f, rec, sp, 1.0, points=rec["pos"][:, :3], dev_points=p4, what="positions as queries")
    own = pkg.shell_host(rec, sp, 1.0)[0]
    assert np.array_equal(q[0]["count"], own["count"] + 1) and q[0]["normal"].tobytes() == own["normal"].tobytes()
    f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (1, 1, 0), (3, 0, 0), (3, 1, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced: the rows are those of the downloaded records, and a later dispatch does not touch them."""
    def check(f, now, sp, what):
        _same(pkg, f, now, sp, what=what)
        return _same(pkg, f, now, sp, _h(sp, 2.0), offset=0.15, what=what)

    def unchanged(f, want):
        _equal(f.shell_rows(), want, "after a dispatch")

    after_dispatches(pkg, kern, aos, graph, check, unchanged)


def test_shell_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    pts = rec["pos"][::5, :3].copy()

    def probe(f):
        f.shell(2.0 * sp.param_h)
        f.query_shell(pts, sp.param_h)

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def _components_held(pkg, f):
    """(labels, roots, table) as the engine holds them now (sph_components_download, no new build)."""
    info = f.component_info()
    n, c = int(info.rows), int(info.numComponents)
    labels, roots, table = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(c, pkg.COMPONENT_DTYPE)
    assert pkg.load_library().sph_components_download(f._h, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), c) == 0
    return labels, roots, table


def test_coexists_with_the_other_queries(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    R = _h(sp, 1.5)
    rays = RS.segments(np.random.default_rng(2), sp, 1024)
    lists, rows, comp, hits = f.neighbors(R), f.knn(16, R), f.components(0.6 * sp.param_h), f.raycast(rays)
    held = _same(pkg, f, rec, sp, R, what="behind the other queries")
    again = f.neighbor_lists()
    assert np.array_equal(again[0], lists[0]) and np.array_equal(again[1], lists[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, f.knn_rows()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(comp, _components_held(pkg, f)))
    RS.same_hits(f.ray_hits(), hits, "after shell()")
    want = pkg.neighbors_host(rec, sp, R)
    assert np.array_equal(lists[0], want[0]) and np.array_equal(lists[1], want[1])
    f.neighbors(_h(sp, 1.0))                                                       # ... and the other way round
    f.knn(8)
    comp2 = f.components(0.6 * sp.param_h)
    f.raycast(rays[:100])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(comp[:3], comp2[:3]))
    _equal(f.shell_rows(), held, "after neighbors(), knn(), components() and raycast()")
    f.close()


def test_python_surface(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(2)
    now = f.download()
    w_rows, w_ids, w_info = pkg.shell_host(now, sp)
    z, ids = f.shell(device=True)
    assert z.is_cuda and z.dtype == torch.float32 and tuple(z.shape) == (len(rec), 8) and ids.is_cuda and ids.dtype == torch.int32
    assert z.cpu().numpy().tobytes() == w_rows.tobytes() and np.array_equal(ids.cpu().numpy(), w_ids)
    assert np.array_equal(z[:, 6].view(torch.int32).cpu().numpy().astype(np.uint32), w_rows["flags"])
    info = f.shell_info()
    rows, hids = f.shell_rows()
    assert info.rows == len(rows) and info.numShell == len(hids) == ((rows["flags"] & pkg.SPH_SHELL_MEMBER) != 0).sum() and info.kind == 1
    assert info.numIsolated == ((rows["flags"] & pkg.SPH_SHELL_ISOLATED) != 0).sum() and info.maxCount == rows["count"].max()
    assert info.radius == F(sp.param_h) and info.stencil == 1 and info.flags == 0
    again = f.shell_rows()
    assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == hids.tobytes()
    a, b = vp(), vp()
    assert pkg.load_library().sph_shell_device(f._h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    dq = f.query_shell(now["pos"][:100, :3], sp.param_h, device=True)
    assert tuple(dq[0].shape) == (100, 8) and dq[0].cpu().numpy().tobytes() == pkg.shell_host(now, sp, points=now["pos"][:100, :3])[0].tobytes()
    f.close()


def test_refusals_and_states(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    info = pkg.SphShellInfo()
    cfg = pkg.shell_config()
    pts = torch.zeros(16, dtype=torch.float32, device="cuda")
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_shell_build(slab._h, C.byref(cfg), C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_shell_query(slab._h, vp(pts.data_ptr()), 4, C.byref(cfg), C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    n = len(rec)
    rows, ids = np.full(n, 9, np.uint8).repeat(32).view(pkg.SHELL_DTYPE), np.full(n, 9, np.int32)
    a, b = vp(), vp()

    def nothing_held():
        assert L.sph_shell_info(f._h, C.byref(info)) == -3
        assert L.sph_shell_device(f._h, C.byref(a), C.byref(b)) == -3
        assert L.sph_shell_download(f._h, rows.ctypes.data_as(vp), ids.ctypes.data_as(vp)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.shell_info()
        assert (ids == 9).all() and (rows.view(np.uint8) == 9).all()
    nothing_held()                                                                 # before any build
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.shell()
        with pytest.raises(pkg.SphError, match="-3"):
            f.query_shell(rec["pos"][:4, :3], sp.param_h)
    nothing_held()
    for bad in (dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=3.01 * sp.param_h), dict(offset=-0.1), dict(offset=float("nan")),
                dict(offset=float("inf")), dict(flags=2), dict(flags=-1)):
        c = pkg.shell_config(**bad)
        assert L.sph_shell_build(f._h, C.byref(c), C.byref(info)) == -1, bad
        assert L.sph_shell_query(f._h, vp(pts.data_ptr()), 4, C.byref(c), C.byref(info)) == -1, bad
    assert L.sph_shell_build(f._h, None, C.byref(info)) == -1 and L.sph_shell_build(f._h, C.byref(cfg), None) == -1
    assert L.sph_shell_build(None, C.byref(cfg), C.byref(info)) == -1
    assert L.sph_shell_query(f._h, None, 4, C.byref(cfg), C.byref(info)) == -1
    assert L.sph_shell_query(f._h, vp(pts.data_ptr()), 1 << 31, C.byref(cfg), C.byref(info)) == -1
    nothing_held()
    want = pkg.shell_host(rec, sp)
    _equal(f.shell(), want, "build")
    bad = pkg.shell_config(offset=-1.0)
    assert L.sph_shell_build(f._h, C.byref(bad), C.byref(info)) == -1              # a refused call leaves the rows alone
    _equal(f.shell_rows(), want, "after a refused call")
    assert L.sph_shell_device(f._h, None, C.byref(b)) == -1 and L.sph_shell_info(f._h, None) == -1
    # null pointers are skipped by the download; device memory is told from host memory by the address
    got_ids = np.zeros(len(want[1]), np.int32)
    assert L.sph_shell_download(f._h, None, got_ids.ctypes.data_as(vp)) == 0 and np.array_equal(got_ids, want[1]) and (rows.view(np.uint8) == 9).all()
    d_rows = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                                       # (the fill runs on torch's stream, the copy on the engine's own)
    assert L.sph_shell_download(f._h, vp(d_rows.data_ptr()), None) == 0 and d_rows.cpu().numpy().tobytes() == want[0].tobytes()
    # the measurement option
    assert f.get_option(pkg.SPH_OPT_SHELL_TIMED) == 0
    for part in (1, 2, 3, 0):
        f.set_option(pkg.SPH_OPT_SHELL_TIMED, part)
        _equal(f.shell(), want, f"SPH_OPT_SHELL_TIMED {part}")
    for v in (-1, 4):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_SHELL_TIMED, v)
    # valid after a dispatch, ended by a reset
    f.DispatchN(2)
    assert f.shell_info().numShell == want[2].numShell
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_shell_particles_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "shell_particles", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "shell_particles OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
