"""Anisotropic kernels on the device (sph_aniso.h) against sph_aniso_host and sph_aniso_lattice_host, byte for byte in the 64-byte rows,
the lattice values and the info, on the smallest shapes where the kernels can go wrong; the surface against the mesher on the twin's
lattice; the interface around them; and the proof that a build changes neither the simulation nor the other query results."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import aniso_scenes as AS
import neighbors_ref as NR
import query_scenes as QS
import rays_scenes as RS
import shell_scenes as SS
from support import after_dispatches, build_example, linked_list_grid, records, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
INFO_FIELDS = ("rows", "numSparse", "numClamped", "maxCount", "radius", "support", "stencil", "maxReach", "reachStencil", "kind", "flags")


def _equal(rows, w_rows, what):
    assert rows.dtype == w_rows.dtype and rows.shape == w_rows.shape, what
    if rows.tobytes() != w_rows.tobytes():
        for key in rows.dtype.names:
            bad = np.flatnonzero((np.ascontiguousarray(rows[key]).view(np.uint32).reshape(len(rows), -1) !=
                                  np.ascontiguousarray(w_rows[key]).view(np.uint32).reshape(len(rows), -1)).any(axis=1))
            assert not len(bad), f"{what}: {key} differs on {len(bad)} of {len(rows)} rows, first {bad[:5].tolist()}: {rows[key][bad[:3]].tolist()} against {w_rows[key][bad[:3]].tolist()}"


def _same(pkg, f, rec, sp, what="", **kw):
    """The device gives sph_aniso_host's bytes and info; returns the host result."""
    want = pkg.aniso_host(rec, sp, **kw)
    _equal(f.anisotropy(**kw), want[0], f"{what} {kw}")
    same_info(f.aniso_info(), want[1], INFO_FIELDS, f"{what} {kw}")
    return want


def _same_lattice(pkg, f, rec, sp, origin, spacing, dims, what="", **kw):
    want, w_info = pkg.aniso_lattice_host(rec, sp, origin, spacing, dims, **kw)
    got = f.aniso_lattice(origin, spacing, dims, **kw)
    assert got.shape == want.shape and got.dtype == F, what
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert not len(bad), f"{what}: {len(bad)} of {got.size} nodes differ, first {bad[:5].tolist()}: {got.ravel()[bad[:3]].tolist()} against {want.ravel()[bad[:3]].tolist()}"
    same_info(f.aniso_info(), w_info, INFO_FIELDS, what)
    return want, w_info


def _h(sp, fac):
    return float(F(fac) * F(sp.param_h))


@pytest.mark.parametrize("fac", [1.0, 1.3, 2.0, 3.0])
def test_edges_of_the_grid(pkg, fac):
    """The uniform box and a cloud up to a quarter of the grid's extent beyond every face (edge, corner and clamped cells), at every
    radius class."""
    rec, sp = QS.uniform(pkg, 3000, seed=31)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rows, info = _same(pkg, f, rec, sp, radius=_h(sp, fac), what="uniform")
    assert info.stencil == int(np.ceil(fac)) and (rows["flags"] & pkg.SPH_ANISO_VALID).all()
    if fac >= 2.0:
        assert info.numSparse < len(rec) // 10
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
    _same(pkg, f, rec, sp, radius=_h(sp, fac), what="clamped")
    f.close()


def test_crowded_cell(pkg):
    """One cell of 300 members among 400 others: long runs of one lane, a run of sorted slots that crosses a block boundary."""
    rec, sp, _, _ = QS.crowded_cell(pkg, 300)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for fac in (1.0, 2.0):
        rows, info = _same(pkg, f, rec, sp, radius=_h(sp, fac), what="crowd")
        assert info.maxCount >= (300 if fac == 2.0 else 100)                       # (within 2h every member of the cell sees all the others, and itself)
    f.close()


def test_special_records(pkg):
    rec, sp = QS.with_ghosts(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    ghost = rec["isGhost"] != 0
    for kw in (dict(), dict(fluid_only=True)):
        for fac in (2.0, 3.0):
            rows, info = _same(pkg, f, rec, sp, radius=_h(sp, fac), what="ghosts", **kw)
            assert ((rows[ghost].view(np.uint8) == 0).all()) == bool(kw)
    f.close()
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    rec["density"][11] = 0.0
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rows, info = _same(pkg, f, rec, sp, what="non-finite")
    assert (rows[[7, 300]].view(np.uint8) == 0).all() and rows["amplitude"][11] == 0 and rows["flags"][11] != 0
    g = QS.grid(pkg, sp)
    _same_lattice(pkg, f, rec, sp, tuple(float(x) for x in g[0]), _h(sp, 0.5), (9, 7, 6), what="non-finite, lattice")
    f.close()
    rec, sp, same = QS.coincident(pkg)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rows, info = _same(pkg, f, rec, sp, what="coincident")
    assert len({rows[i].tobytes() for i in same}) == 1
    f.close()
    # degenerate neighbourhoods: every interior row of the layer and every row of the line is clamped
    for scene, kw in ((AS.layer(pkg), dict()), (AS.line(pkg), dict(min_count=4))):
        f = pkg.SPHFluidGPU.from_particles(scene[0], scene[1])
        rows, info = _same(pkg, f, scene[0], scene[1], what="degenerate", **kw)
        assert info.numClamped > 30
        f.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_tiny_engines(pkg, n):
    sp = QS.params(pkg)
    rec = QS.uniform(pkg, max(n, 1), seed=5)[0][:n]
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rows, info = _same(pkg, f, rec, sp, what=f"n = {n}")
    assert info.kind == 1 and info.rows == n
    if n == 1:
        assert rows["count"].tolist() == [1] and rows["flags"].tolist() == [3]
    _same(pkg, f, rec, sp, min_count=0, max_ratio=1.0, what=f"n = {n}, spheres by the clamp")
    g = QS.grid(pkg, sp)
    want, w_info = _same_lattice(pkg, f, rec, sp, tuple(float(x) for x in g[0]), _h(sp, 0.5), (17, 13, 15), what=f"n = {n}, lattice")
    assert (np.count_nonzero(want) > 0) if n >= 63 else (n > 0 or (want == 0).all())
    f.close()


def test_lattices_on_the_ball(pkg):
    """The ball of 5 spacings at spacing h / 2: one node, partial bricks, the bar that overhangs the grid, a NaN origin component, an
    empty lattice; and a cloud beyond the grid's faces under a lattice that overhangs every face."""
    rec, sp, _ = SS.ball(pkg, 5.0)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    s = _h(sp, 0.5)
    want, _ = _same_lattice(pkg, f, rec, sp, (0.01, -0.02, 0.03), s, (1, 1, 1), what="one node")
    assert want[0, 0, 0] > 1.0
    want, _ = _same_lattice(pkg, f, rec, sp, (-4 * s, -4 * s, -2 * s), s, (9, 8, 5), what="partial bricks")
    assert np.count_nonzero(want) > 150
    origin, spacing, dims = AS.ball_lattice(pkg, sp, overhang=True)
    want, _ = _same_lattice(pkg, f, rec, sp, origin, spacing, dims, what="overhang")
    assert np.count_nonzero(want) > 200 and (want[:, :, 0] == 0).all()
    want, _ = _same_lattice(pkg, f, rec, sp, (float("nan"), -4 * s, -2 * s), s, (9, 8, 5), what="NaN origin")
    assert (want == 0).all() and not np.signbit(want).any()
    want, _ = _same_lattice(pkg, f, rec, sp, (-4 * s, float("inf"), -2 * s), s, (3, 3, 3), what="inf origin")
    assert (want == 0).all()
    got = f.aniso_lattice((0, 0, 0), s, (4, 0, 4))
    assert got.shape == (4, 0, 4) and f.aniso_info().rows == len(rec)
    dev = f.aniso_lattice((-4 * s, -4 * s, -2 * s), s, (9, 8, 5), device=True)
    assert dev.is_cuda and tuple(dev.shape) == (5, 8, 9)
    assert dev.cpu().numpy().tobytes() == pkg.aniso_lattice_host(rec, sp, (-4 * s, -4 * s, -2 * s), s, (9, 8, 5))[0].tobytes()
    # the isotropic limit on the device too
    _same_lattice(pkg, f, rec, sp, (-4 * s, -4 * s, -2 * s), s, (9, 8, 5), min_count=2 ** 32 - 1, sparse_scale=1.0, smoothing=0.0, support=sp.param_h,
                  what="spheres of radius h")
    f.close()
    sp = QS.params(pkg)
    grid = QS.grid(pkg, sp)
    lo, gd, cs = grid
    pos = QS.grid_cloud(np.random.default_rng(4), grid, 2500, beyond=0.25)
    rec = records(pkg, pos, np.zeros_like(pos))
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    s = _h(sp, 0.5)
    origin = tuple(float(x) for x in lo - F(0.3) * gd.astype(F) * cs)
    dims = tuple(int(np.ceil(1.6 * float(gd[a]) * float(cs) / s)) + 1 for a in range(3))
    want, info = _same_lattice(pkg, f, rec, sp, origin, s, dims, what="clamped cells")
    assert np.count_nonzero(want) > 1000 and info.reachStencil >= 2
    f.close()


def _closed(tris, nv):
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64), axis=1)
    assert (e[:, 0] != e[:, 1]).all() and e.max() < nv
    _, counts = np.unique(e[:, 0] * nv + e[:, 1], return_counts=True)
    return (counts == 2).all()


def test_surface_is_the_mesh_of_the_twins_lattice(pkg):
    import torch
    rec, sp, _ = SS.ball(pkg, 5.0)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    origin, spacing, dims = AS.ball_lattice(pkg, sp)
    bulk = float(pkg.aniso_lattice_host(rec, sp, (0, 0, 0), 0.1, (1, 1, 1))[0][0, 0, 0])
    for kw in (dict(), dict(smoothing=0.5, max_ratio=2.0)):
        vol, info = pkg.aniso_lattice_host(rec, sp, origin, spacing, dims, **kw)
        v, t = f.aniso_surface(origin, spacing, dims, iso=0.5 * bulk, **kw)
        same_info(f.aniso_info(), info, INFO_FIELDS, "surface")
        wv, wt = f.surface_from_volume(torch.from_numpy(vol).cuda(), origin, spacing, iso=0.5 * bulk)
        assert len(v) > 100 and len(t) > 200 and v.tobytes() == wv.tobytes() and t.tobytes() == wt.tobytes()
        assert _closed(t, len(v))
        sv, st = f.surface(origin, spacing, dims, iso=2.0)                         # the isotropic surface is as ever, and another one
        assert len(sv) > 100 and _closed(st, len(sv)) and sv.tobytes() != v.tobytes()
    # the default lattice
    v, t = f.aniso_surface(iso=0.5 * bulk)
    o, s, d = f.default_surface_lattice()
    wv, wt = f.surface_from_volume(torch.from_numpy(pkg.aniso_lattice_host(rec, sp, o, s, d)[0]).cuda(), o, s, iso=0.5 * bulk)
    assert len(v) > 100 and v.tobytes() == wv.tobytes() and t.tobytes() == wt.tobytes() and _closed(t, len(v))
    f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (1, 1, 0), (3, 0, 0), (3, 1, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced: rows and lattice are those of the downloaded records (1/rho of the sorted copy is 1 / density of
    the record), and a later dispatch does not touch the rows."""
    def check(f, now, sp, what):
        g = QS.grid(pkg, sp)
        _same_lattice(pkg, f, now, sp, tuple(float(x) for x in g[0]), _h(sp, 0.5), (17, 9, 12), what=what)
        _same(pkg, f, now, sp, radius=_h(sp, 1.5), support=_h(sp, 0.8), smoothing=0.5, what=what)
        return _same(pkg, f, now, sp, what=what)

    def unchanged(f, want):
        _equal(f.aniso_rows(), want[0], "after a dispatch")

    after_dispatches(pkg, kern, aos, graph, check, unchanged)


def test_aniso_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    g = QS.grid(pkg, sp)
    origin = tuple(float(x) for x in g[0])

    def probe(f):
        f.anisotropy()
        f.aniso_lattice(origin, sp.param_h, (8, 8, 8))
        f.aniso_surface(origin, sp.param_h, (8, 8, 8))

    for aos, graph in ((1, 0), (0, 0), (1, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def _components_held(pkg, f):
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
    lists, rows, comp, hits, shell = f.neighbors(R), f.knn(16, R), f.components(0.6 * sp.param_h), f.raycast(rays), f.shell(R)
    held = _same(pkg, f, rec, sp, what="behind the other queries")
    g = QS.grid(pkg, sp)
    f.aniso_surface(tuple(float(x) for x in g[0]), sp.param_h, (8, 8, 8))
    again = f.neighbor_lists()
    assert np.array_equal(again[0], lists[0]) and np.array_equal(again[1], lists[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, f.knn_rows()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(comp, _components_held(pkg, f)))
    RS.same_hits(f.ray_hits(), hits, "after anisotropy()")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(shell, f.shell_rows()))
    f.neighbors(_h(sp, 1.0))                                                       # ... and the other way round
    f.knn(8)
    f.components(0.6 * sp.param_h)
    f.raycast(rays[:100])
    f.shell()
    f.surface()
    _equal(f.aniso_rows(), held[0], "after neighbors(), knn(), components(), raycast(), shell() and surface()")
    f.close()


def test_python_surface(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(2)
    now = f.download()
    w_rows, w_info = pkg.aniso_host(now, sp)
    z = f.anisotropy(device=True)
    assert z.is_cuda and z.dtype == torch.float32 and tuple(z.shape) == (len(rec), 16)
    assert z.cpu().numpy().tobytes() == w_rows.tobytes()
    assert np.array_equal(z[:, 7].view(torch.int32).cpu().numpy().astype(np.uint32), w_rows["flags"])
    info = f.aniso_info()
    rows = f.aniso_rows()
    assert info.rows == len(rows) and info.kind == 1 and info.numSparse == ((rows["flags"] & pkg.SPH_ANISO_SPARSE) != 0).sum()
    assert info.numClamped == ((rows["flags"] & pkg.SPH_ANISO_CLAMPED) != 0).sum() and info.maxCount == rows["count"].max() and info.maxReach == rows["reach"].max()
    assert info.radius == F(2) * F(sp.param_h) and info.support == F(sp.param_h) and info.stencil == 2 and info.flags == 0
    assert f.aniso_rows().tobytes() == rows.tobytes()
    a = vp()
    assert pkg.load_library().sph_aniso_device(f._h, C.byref(a)) == 0 and a.value
    f.close()


def test_refusals_and_states(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    info, surf = pkg.SphAnisoInfo(), pkg.SphSurface()
    cfg = pkg.aniso_config()
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    o3, s3, d3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int * 3)(4, 4, 4)
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_aniso_build(slab._h, C.byref(cfg), C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_aniso_lattice(slab._h, C.byref(cfg), o3, s3, d3, vp(out.data_ptr()), C.byref(info)) == -3
        assert L.sph_aniso_surface(slab._h, C.byref(cfg), o3, s3, d3, 0.5, C.byref(surf), C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    n = len(rec)
    rows = np.full(n, 9, np.uint8).repeat(64).view(pkg.ANISO_DTYPE)
    a = vp()

    def nothing_held():
        assert L.sph_aniso_info(f._h, C.byref(info)) == -3
        assert L.sph_aniso_device(f._h, C.byref(a)) == -3
        assert L.sph_aniso_download(f._h, rows.ctypes.data_as(vp)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.aniso_info()
        assert (rows.view(np.uint8) == 9).all()
    nothing_held()                                                                 # before any build
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.anisotropy()
        with pytest.raises(pkg.SphError, match="-3"):
            f.aniso_lattice((0, 0, 0), 0.1, (4, 4, 4))
        with pytest.raises(pkg.SphError, match="-3"):
            f.aniso_surface()
    nothing_held()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=nan), dict(radius=inf), dict(radius=3.01 * sp.param_h), dict(support=nan), dict(support=inf), dict(smoothing=-0.1),
                dict(smoothing=1.5), dict(smoothing=nan), dict(maxRatio=0.5), dict(maxRatio=inf), dict(maxStretch=0.0), dict(maxStretch=nan),
                dict(sparseScale=0.0), dict(sparseScale=inf), dict(flags=2), dict(flags=-1)):
        c = pkg.aniso_config(**bad)
        assert L.sph_aniso_build(f._h, C.byref(c), C.byref(info)) == -1, bad
        assert L.sph_aniso_lattice(f._h, C.byref(c), o3, s3, d3, vp(out.data_ptr()), C.byref(info)) == -1, bad
        assert L.sph_aniso_surface(f._h, C.byref(c), o3, s3, d3, 0.5, C.byref(surf), C.byref(info)) == -1, bad
    assert L.sph_aniso_build(f._h, None, C.byref(info)) == -1 and L.sph_aniso_build(f._h, C.byref(cfg), None) == -1
    assert L.sph_aniso_build(None, C.byref(cfg), C.byref(info)) == -1
    assert L.sph_aniso_lattice(f._h, C.byref(cfg), o3, s3, d3, None, C.byref(info)) == -1
    assert L.sph_aniso_lattice(f._h, C.byref(cfg), o3, s3, (C.c_int * 3)(4, -1, 4), vp(out.data_ptr()), C.byref(info)) == -1
    assert L.sph_aniso_lattice(f._h, C.byref(cfg), o3, (C.c_float * 3)(0.1, 0.0, 0.1), d3, vp(out.data_ptr()), C.byref(info)) == -1
    assert L.sph_aniso_surface(f._h, C.byref(cfg), o3, s3, (C.c_int * 3)(4, 1, 4), 0.5, C.byref(surf), C.byref(info)) == -1     # (the mesher needs two nodes per axis)
    assert L.sph_aniso_surface(f._h, C.byref(cfg), o3, s3, d3, nan, C.byref(surf), C.byref(info)) == -1
    assert L.sph_aniso_surface(f._h, C.byref(cfg), o3, s3, d3, 0.5, None, C.byref(info)) == -1
    nothing_held()
    want = pkg.aniso_host(rec, sp)
    _equal(f.anisotropy(), want[0], "build")
    bad = pkg.aniso_config(smoothing=2.0)
    assert L.sph_aniso_build(f._h, C.byref(bad), C.byref(info)) == -1              # a refused call leaves the rows alone
    _equal(f.aniso_rows(), want[0], "after a refused call")
    assert L.sph_aniso_device(f._h, None) == -1 and L.sph_aniso_info(f._h, None) == -1
    d_rows = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                                       # (the fill runs on torch's stream, the copy on the engine's own)
    assert L.sph_aniso_download(f._h, vp(d_rows.data_ptr())) == 0 and d_rows.cpu().numpy().tobytes() == want[0].tobytes()
    assert L.sph_aniso_download(f._h, None) == 0
    # the three-cell refusal names maxReach and still holds the rows of that build
    wide = dict(support=3.1 * sp.param_h)
    with pytest.raises(pkg.SphError, match="-1.*maxReach"):
        f.aniso_lattice((0, 0, 0), 0.1, (4, 4, 4), **wide)
    held = f.aniso_info()
    assert held.reachStencil == 0 and held.maxReach > 3 * sp.param_h and held.support == F(3.1 * sp.param_h)
    _equal(f.aniso_rows(), pkg.aniso_host(rec, sp, **wide)[0], "the rows of the refused lattice")
    with pytest.raises(pkg.SphError, match="-1.*maxReach"):
        f.aniso_surface(**wide)
    with pytest.raises(pkg.SphError, match="no surface|-3"):
        f._download_surface(pkg.SphSurface())
    # valid after a dispatch, ended by a reset
    f.anisotropy()
    f.DispatchN(2)
    assert f.aniso_info().numClamped == want[1].numClamped
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_aniso_surface_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "aniso_surface", tmp_path, werror=True), ["20000", "2"], timeout=120)
    assert res.returncode == 0 and "aniso_surface OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 2
