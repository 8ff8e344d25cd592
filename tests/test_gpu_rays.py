"""Ray casts on the device (sph_rays.h) against sph_rays_host, the brute-force definition, byte for byte in t, id, pos and normal and in
the counts, on the smallest shapes where a grid walk can go wrong (rays_scenes.scenes: rays along cell faces and edges and through cell
corners, zero direction components, starts outside the box, spheres that stick out of it, clamped records, r = half a cell exactly, a
dense lattice, ties); the interface around it; and the proof that a cast changes neither the simulation nor the other query results."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import rays_scenes as RS
from support import build_example, linked_list_grid, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
INFO_FIELDS = ("rays", "hits", "voidRays", "radius", "flags")


def _same(pkg, f, rec, sp, r, radius, what, dev=False, **kw):
    """Both variants (rays cast in the caller's order, and in the order of their cell of entry) give the definition's bytes and counts;
    returns the host result."""
    want = pkg.rays_host(rec, sp, r, radius, with_info=True, **kw)
    for variant in (0, 1):
        f.set_option(pkg.SPH_OPT_RAYS_VARIANT, variant)
        if dev:
            import torch
            got = f.raycast(torch.from_numpy(np.ascontiguousarray(r)).cuda(), radius, **kw)
        else:
            got = f.raycast(r, radius, **kw)
        RS.same_hits(got, want, f"{what} variant {variant}")
        same_info(f.rays_info(), want[4], INFO_FIELDS, what)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 0)
    return want


SCENES = None


def _scenes(pkg):
    global SCENES
    if SCENES is None:
        SCENES = RS.scenes(pkg)
    return SCENES


@pytest.mark.parametrize("which", range(8))
def test_scene_against_the_definition(pkg, which):
    """Every scene, every cast of it, through sph_rays_cast and sph_rays_cast_device."""
    assert len(_scenes(pkg)) == 8                                                  # (the parametrisation covers every scene)
    name, rec, sp, casts = _scenes(pkg)[which]
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    hits = 0
    for j, (r, radius, kw) in enumerate(casts):
        want = _same(pkg, f, rec, sp, r, radius, f"{name} cast {j} r {radius} {kw}", **kw)
        _same(pkg, f, rec, sp, r, radius, f"{name} cast {j} r {radius} {kw} (device rays)", dev=True, **kw)
        hits += int(want[4].hits)
    assert hits > 0
    f.close()


def test_default_radius_and_empty_engines(pkg):
    rec, sp = RS.uniform(pkg, 300, 41)
    r = RS.segments(np.random.default_rng(3), sp, 257)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    RS.same_hits(f.raycast(r), pkg.rays_host(rec, sp, r, 0.25 * sp.param_h), "radius None: h / 4")
    t, ids, pos, nrm = f.raycast(r[:0])                                            # m = 0
    assert t.shape == (0,) and ids.shape == (0,) and pos.shape == (0, 3) and f.rays_info().rays == 0 and f.rays_info().hits == 0
    f.close()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)                                         # n = 0: every ray a miss, void rays still counted
    f = pkg.SPHFluidGPU.from_particles(none, sp)
    _same(pkg, f, none, sp, RS.void_mix(r, np.random.default_rng(4)), 0.25, "n = 0")
    assert f.rays_info().hits == 0 and f.rays_info().voidRays > 0
    f.close()


@pytest.mark.parametrize("aos", [1, 0])
def test_after_reset_and_substeps(pkg, aos):
    """The default spawn after sph_reset and 8 substeps: a sheet straight down and a pinhole fan from a corner, against the definition on
    the downloaded records; a later dispatch does not touch the hits."""
    f = pkg.SPHFluidGPU(6000)
    f.set_option(pkg.SPH_OPT_AOS_MODE, aos)
    f.ResetSimulation()
    f.DispatchN(8)
    now, sp = f.download(), f.params
    g = pkg.compute_grid_extents(sp)
    lo, ext = np.array(list(g.gridMin), F), np.array(list(g.dims), F) * F(g.cellSize)
    sheet = pkg.parallel_rays((lo[0], lo[1] + ext[1] + 1.0, lo[2]), (ext[0], 0, 0), (0, 0, ext[2]), (0, -1, 0), 48, 48)
    fan = pkg.camera_rays(lo + ext * F(1.3), lo + ext * F(0.5), (0, 1, 0), 0.9, 64, 48)
    r = np.concatenate([sheet, fan])
    want = _same(pkg, f, now, sp, r, 0.25 * sp.param_h, f"aos {aos}")
    assert want[4].hits > 100
    _same(pkg, f, now, sp, r, 0.5 * sp.param_h, f"aos {aos}, r = h / 2", fluid_only=True)
    held = f.ray_hits()
    f.DispatchN(2)
    RS.same_hits(f.ray_hits(), held, "after a dispatch")
    f.close()


def test_device_tensors(pkg):
    import torch
    rec, sp = RS.uniform(pkg, 1200, 42)
    r = RS.segments(np.random.default_rng(9), sp, 1000)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    t, ids, pos, nrm = f.raycast(r, 0.25, device=True)
    assert t.is_cuda and t.dtype == torch.float32 and ids.dtype == torch.int32 and tuple(pos.shape) == (1000, 3) == tuple(nrm.shape)
    RS.same_hits([x.cpu().contiguous().numpy() for x in (t, ids, pos, nrm)], f.ray_hits(), "device tensors against the download")
    RS.same_hits(f.ray_hits(), pkg.rays_host(rec, sp, r, 0.25), "download")
    p = vp()
    assert pkg.load_library().sph_rays_device(f._h, C.byref(p)) == 0 and p.value
    f.close()


def test_coexists_with_neighbour_lists_and_knn(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    R = float(F(1.5) * F(sp.param_h))
    lists, rows = f.neighbors(R), f.knn(16, R)
    r = RS.segments(np.random.default_rng(2), sp, 1024)
    held = _same(pkg, f, rec, sp, r, 0.25 * sp.param_h, "between the queries")
    again, rows2 = f.neighbor_lists(), f.knn_rows()
    assert np.array_equal(again[0], lists[0]) and np.array_equal(again[1], lists[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, rows2))
    f.neighbors(float(sp.param_h))                                                 # ... and the other way round
    f.knn(8)
    f.components(0.6 * sp.param_h)
    RS.same_hits(f.ray_hits(), held, "after neighbors(), knn() and components()")
    f.close()


def test_a_cast_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    r = RS.segments(np.random.default_rng(6), sp, 2048)

    def probe(f):
        f.raycast(r)
        f.raycast(r[:500], 0.5 * sp.param_h, any_hit=True)

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
    info = pkg.SphRaysInfo()
    r = RS.segments(np.random.default_rng(8), sp, 16)
    dr = torch.from_numpy(r).cuda()
    rad = float(F(0.25) * F(sp.param_h))
    cs = float(pkg.compute_grid_extents(sp).cellSize)
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_rays_cast(slab._h, r.ctypes.data_as(vp), 16, rad, 0, C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_rays_cast_device(slab._h, vp(dr.data_ptr()), 16, rad, 0, C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    hits = np.full(16, 9, np.int32).repeat(8).view(pkg.RAY_HIT_DTYPE)
    p = vp()

    def nothing_held():
        assert L.sph_rays_info(f._h, C.byref(info)) == -3 and L.sph_rays_device(f._h, C.byref(p)) == -3
        assert L.sph_rays_download(f._h, hits.ctypes.data_as(vp)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.rays_info()
        assert (hits["id"] == 9).all()
    nothing_held()                                                                 # before any cast
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.raycast(r)
        with pytest.raises(pkg.SphError, match="-3"):
            f.raycast(dr)
    nothing_held()
    for bad in (0.0, -1.0, float("nan"), float("inf"), float(np.nextafter(F(0.5) * F(cs), F(9)))):
        assert L.sph_rays_cast(f._h, r.ctypes.data_as(vp), 16, bad, 0, C.byref(info)) == -1
        assert L.sph_rays_cast_device(f._h, vp(dr.data_ptr()), 16, bad, 0, C.byref(info)) == -1
    assert L.sph_rays_cast(f._h, r.ctypes.data_as(vp), 16, rad, 4, C.byref(info)) == -1        # an unknown flag bit
    assert L.sph_rays_cast(f._h, None, 16, rad, 0, C.byref(info)) == -1 and L.sph_rays_cast(f._h, r.ctypes.data_as(vp), 16, rad, 0, None) == -1
    assert L.sph_rays_cast(None, r.ctypes.data_as(vp), 16, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_cast_device(f._h, None, 16, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_cast_device(f._h, vp(dr.data_ptr()), 1 << 31, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_cast(f._h, r.ctypes.data_as(vp), 1 << 31, rad, 0, C.byref(info)) == -1
    with pytest.raises(pkg.SphError):
        f.raycast(np.zeros((4, 7), F))
    with pytest.raises(pkg.SphError):
        f.raycast(dr[:, :7])
    nothing_held()
    want = pkg.rays_host(rec, sp, r, rad)
    RS.same_hits(f.raycast(r, rad), want, "cast")
    RS.same_hits(f.raycast(r, float(F(0.5) * F(cs))), pkg.rays_host(rec, sp, r, float(F(0.5) * F(cs))), "half a cell exactly")
    f.raycast(r, rad)
    assert L.sph_rays_cast(f._h, r.ctypes.data_as(vp), 16, rad, 4, C.byref(info)) == -1        # a refused call leaves the hits alone
    RS.same_hits(f.ray_hits(), want, "after a refused call")
    assert L.sph_rays_device(f._h, None) == -1 and L.sph_rays_info(f._h, None) == -1 and L.sph_rays_download(f._h, None) == -1
    d_hits = torch.empty((16, 8), dtype=torch.float32, device="cuda")               # device memory is told from host memory by the address
    torch.cuda.synchronize()                                                       # (nothing of the caller's is queued on the array: the copy runs on the engine's stream)
    assert L.sph_rays_download(f._h, vp(d_hits.data_ptr())) == 0
    assert d_hits.cpu().numpy()[:, 0].tobytes() == want[0].tobytes()
    assert f.get_option(pkg.SPH_OPT_RAYS_VARIANT) == 0                             # the option
    for bad in (-1, 2):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_RAYS_VARIANT, bad)
    f.DispatchN(2)                                                                 # valid after a dispatch, ended by a reset
    assert f.rays_info().rays == 16
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_range_scan_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "range_scan", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "range_scan OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
