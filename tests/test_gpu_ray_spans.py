"""Ray spans on the device (k_ray_spans of sph_rays.h) against sph_rays_span_host, the brute-force definition, byte for byte in every
field of the 32-byte rows and in the counts: on every scene of rays_scenes.py, for both span walks (SPH_OPT_RAY_SPANS_VARIANT) and both
ray orders (SPH_OPT_RAYS_VARIANT), with host arrays and with device tensors; the interface around it; and the proof that a span call
changes neither the simulation nor the hits held from a cast."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import ray_spans_ref as SR
import rays_scenes as RS
from support import build_example, linked_list_grid, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p


def _rows(pkg, z):
    """What ray_spans returns as RAY_SPAN_DTYPE rows: a device tensor of (m, 8) int32 holds the same bytes."""
    if isinstance(z, np.ndarray):
        return z
    return np.ascontiguousarray(z.cpu().numpy()).view(pkg.RAY_SPAN_DTYPE).reshape(-1)


def _same(pkg, f, rec, sp, r, radius, what, dev=False, **kw):
    """Both span walks in both ray orders give the definition's bytes and counts; returns the host result (rows, info)."""
    want, info = pkg.ray_spans_host(rec, sp, r, radius, with_info=True, **kw)
    SR.info_of_rows(want, info, what)
    for walk in (0, 1):
        for order in (0, 1):
            f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, walk)
            f.set_option(pkg.SPH_OPT_RAYS_VARIANT, order)
            if dev:
                import torch
                got = _rows(pkg, f.ray_spans(torch.from_numpy(np.ascontiguousarray(r)).cuda(), radius, device=True, **kw))
            else:
                got = f.ray_spans(r, radius, **kw)
            SR.same_rows(got, want, f"{what} walk {walk} order {order}")
            same_info(f.ray_spans_info(), info, SR.INFO_FIELDS, f"{what} walk {walk} order {order}")
    f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, 0)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 0)
    return want, info


@pytest.mark.parametrize("which", range(8))
def test_scene_against_the_definition(pkg, which):
    """Every scene, every set of rays of it, through sph_rays_span and sph_rays_span_device; on the `far` and `lat` families the first
    entry is the cast's first hit (ray_spans_ref.first_entry)."""
    assert len(SR.scenes(pkg)) == 8                                                # (the parametrisation covers every scene)
    name, rec, sp, casts = SR.scenes(pkg)[which]
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    crossed = 0
    for j, (r, radius, kw) in enumerate(casts):
        what = f"{name} rays {j} r {radius} {kw}"
        want, info = _same(pkg, f, rec, sp, r, radius, what, **kw)
        _same(pkg, f, rec, sp, r, radius, what + " (device rays)", dev=True, **kw)
        if SR.far_or_lat(pkg, r):
            SR.first_entry(pkg, rec, sp, r, radius, f.ray_span_rows(), f.raycast(r, radius, **kw), what, exact=name == "uniform 1200")
        crossed += int(info.crossed)
    assert crossed > 0
    f.close()


def test_default_radius_and_empty_engines(pkg):
    rec, sp = RS.uniform(pkg, 300, 41)
    r = RS.segments(np.random.default_rng(3), sp, 257)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    SR.same_rows(f.ray_spans(r), pkg.ray_spans_host(rec, sp, r, 0.25 * sp.param_h), "radius None: h / 4")
    rows = f.ray_spans(r[:0])                                                      # m = 0
    info = f.ray_spans_info()
    assert rows.shape == (0,) and rows.dtype == pkg.RAY_SPAN_DTYPE and (info.rays, info.crossed, info.total, info.maxCount) == (0, 0, 0, 0)
    assert tuple(f.ray_spans(r[:0], device=True).shape) == (0, 8)
    f.close()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)                                         # n = 0: nothing is crossed, void rays still counted
    f = pkg.SPHFluidGPU.from_particles(none, sp)
    _same(pkg, f, none, sp, RS.void_mix(r, np.random.default_rng(4)), 0.25, "n = 0")
    assert f.ray_spans_info().crossed == 0 and f.ray_spans_info().voidRays > 0
    f.close()


@pytest.mark.parametrize("aos", [1, 0])
def test_after_reset_and_substeps(pkg, aos):
    """The default spawn after sph_reset and 8 substeps: a sheet straight down and a pinhole fan from a corner, against the definition on
    the downloaded records; a later dispatch does not touch the spans."""
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
    want, info = _same(pkg, f, now, sp, r, 0.25 * sp.param_h, f"aos {aos}")
    assert info.crossed > 100 and info.maxCount > 1
    _same(pkg, f, now, sp, r, 0.5 * sp.param_h, f"aos {aos}, r = h / 2", fluid_only=True)
    held = f.ray_span_rows()
    f.DispatchN(2)
    SR.same_rows(f.ray_span_rows(), held, "after a dispatch")
    f.close()


def test_device_tensors(pkg):
    import torch
    rec, sp = RS.uniform(pkg, 1200, 42)
    r = RS.segments(np.random.default_rng(9), sp, 1000)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    z = f.ray_spans(r, 0.25, device=True)
    assert z.is_cuda and z.dtype == torch.int32 and tuple(z.shape) == (1000, 8)
    SR.same_rows(_rows(pkg, z), f.ray_span_rows(), "device tensor against the download")
    SR.same_rows(f.ray_span_rows(), pkg.ray_spans_host(rec, sp, r, 0.25), "download")
    p = vp()
    assert pkg.load_library().sph_rays_span_rows(f._h, C.byref(p)) == 0 and p.value
    f.close()


def test_spans_and_hits_are_separate_state(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    r = RS.segments(np.random.default_rng(2), sp, 1024)
    rad = 0.25 * sp.param_h
    hits = f.raycast(r, rad)
    RS.same_hits(hits, pkg.rays_host(rec, sp, r, rad), "cast")
    rows = f.ray_spans(r[:700], 0.5 * sp.param_h)                                  # other rays, another radius
    SR.same_rows(rows, pkg.ray_spans_host(rec, sp, r[:700], 0.5 * sp.param_h), "spans")
    RS.same_hits(f.ray_hits(), hits, "the hits after a span call")
    assert f.rays_info().rays == 1024 and f.ray_spans_info().rays == 700
    f.raycast(r[:300], rad, any_hit=True)                                          # ... and the other way round
    SR.same_rows(f.ray_span_rows(), rows, "the spans after a cast")
    assert f.rays_info().rays == 300 and f.ray_spans_info().rays == 700
    f.neighbors(float(sp.param_h))
    f.knn(8)
    SR.same_rows(f.ray_span_rows(), rows, "after neighbors() and knn()")
    f.close()


def test_a_span_call_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    r = RS.segments(np.random.default_rng(6), sp, 2048)

    def probe(f):
        f.ray_spans(r)
        f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, 1)
        f.ray_spans(r[:500], 0.5 * sp.param_h, fluid_only=True)
        f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, 0)

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
    info = pkg.SphRaySpansInfo()
    r = RS.segments(np.random.default_rng(8), sp, 16)
    dr = torch.from_numpy(r).cuda()
    rad = float(F(0.25) * F(sp.param_h))
    cs = float(pkg.compute_grid_extents(sp).cellSize)
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_rays_span(slab._h, r.ctypes.data_as(vp), 16, rad, 0, C.byref(info)) == -3 and b"slab" in L.sph_last_error()
        assert L.sph_rays_span_device(slab._h, vp(dr.data_ptr()), 16, rad, 0, C.byref(info)) == -3
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    rows = np.full(16, 9, np.int32).repeat(8).view(pkg.RAY_SPAN_DTYPE)
    p = vp()

    def nothing_held():
        assert L.sph_rays_span_info(f._h, C.byref(info)) == -3 and L.sph_rays_span_rows(f._h, C.byref(p)) == -3
        assert L.sph_rays_span_download(f._h, rows.ctypes.data_as(vp)) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.ray_spans_info()
        with pytest.raises(pkg.SphError, match="-3"):
            f.ray_span_rows()
        assert (rows["idEnter"] == 9).all()
    nothing_held()                                                                 # before any call
    f.raycast(r, rad)                                                              # (a cast gives hits, not spans)
    nothing_held()
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.ray_spans(r)
        with pytest.raises(pkg.SphError, match="-3"):
            f.ray_spans(dr)
    nothing_held()
    for bad in (0.0, -1.0, float("nan"), float("inf"), float(np.nextafter(F(0.5) * F(cs), F(9)))):
        assert L.sph_rays_span(f._h, r.ctypes.data_as(vp), 16, bad, 0, C.byref(info)) == -1
        assert L.sph_rays_span_device(f._h, vp(dr.data_ptr()), 16, bad, 0, C.byref(info)) == -1
    for flags in (pkg.SPH_RAYS_ANY_HIT, pkg.SPH_RAYS_ANY_HIT | pkg.SPH_RAYS_FLUID_ONLY, 4):  # any_hit has no meaning here; an unknown bit
        assert L.sph_rays_span(f._h, r.ctypes.data_as(vp), 16, rad, flags, C.byref(info)) == -1
        assert L.sph_rays_span_device(f._h, vp(dr.data_ptr()), 16, rad, flags, C.byref(info)) == -1
    assert L.sph_rays_span(f._h, None, 16, rad, 0, C.byref(info)) == -1 and L.sph_rays_span(f._h, r.ctypes.data_as(vp), 16, rad, 0, None) == -1
    assert L.sph_rays_span(None, r.ctypes.data_as(vp), 16, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_span_device(f._h, None, 16, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_span_device(f._h, vp(dr.data_ptr()), 1 << 31, rad, 0, C.byref(info)) == -1
    assert L.sph_rays_span(f._h, r.ctypes.data_as(vp), 1 << 31, rad, 0, C.byref(info)) == -1
    with pytest.raises(pkg.SphError):
        f.ray_spans(np.zeros((4, 7), F))
    with pytest.raises(pkg.SphError):
        f.ray_spans(dr[:, :7])
    nothing_held()
    want = pkg.ray_spans_host(rec, sp, r, rad)
    SR.same_rows(f.ray_spans(r, rad), want, "spans")
    half = float(F(0.5) * F(cs))
    SR.same_rows(f.ray_spans(r, half), pkg.ray_spans_host(rec, sp, r, half), "half a cell exactly")
    f.ray_spans(r, rad)
    assert L.sph_rays_span(f._h, r.ctypes.data_as(vp), 16, rad, 4, C.byref(info)) == -1        # a refused call leaves the spans alone
    SR.same_rows(f.ray_span_rows(), want, "after a refused call")
    assert L.sph_rays_span_rows(f._h, None) == -1 and L.sph_rays_span_info(f._h, None) == -1 and L.sph_rays_span_download(f._h, None) == -1
    d_rows = torch.empty((16, 8), dtype=torch.int32, device="cuda")                 # device memory is told from host memory by the address
    torch.cuda.synchronize()                                                       # (nothing of the caller's is queued on the array: the copy runs on the engine's stream)
    assert L.sph_rays_span_download(f._h, vp(d_rows.data_ptr())) == 0
    SR.same_rows(_rows(pkg, d_rows), want, "download into device memory")
    assert f.get_option(pkg.SPH_OPT_RAY_SPANS_VARIANT) == 0                        # the option: the layer walk is the default
    for bad in (-1, 2):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, bad)
    f.DispatchN(2)                                                                 # valid after a dispatch, ended by a reset
    assert f.ray_spans_info().rays == 16
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_column_depth_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "column_depth", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "column_depth OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
