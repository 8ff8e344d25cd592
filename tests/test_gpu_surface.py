"""Iso-surface meshes on the GPU (include/sph_abi.h "iso-surface"): byte-for-byte equality with the numpy
restatement of tests/surface_ref.py on volumes and on sampled fields, the settled pool's closed surface and volume, no effect on the
simulation, repeatability, refusals, the C++ example and one full-size case."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT, assert_records_equal, small_scene
import surface_ref as sr
from support import build_example, run_example, undisturbed_run

pytestmark = pytest.mark.gpu

G = os.path.join(ROOT, "tests", "golden")
F = np.float32


def _want(pkg, f, origin, spacing, iso):
    pos, nrm, tris = sr.extract(f, origin, spacing, iso)
    v = np.zeros(len(pos), pkg.SURFACE_VERTEX_DTYPE)
    v["pos"], v["normal"] = pos, nrm
    return v, tris


def _volume_surface(pkg, eng, f, origin, spacing, iso):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(f, F)).cuda()
    return eng.surface_from_volume(t, origin, spacing, None, iso)


def _assert_same(pkg, got, want, what):
    gv, gt = got
    wv, wt = want
    assert len(gv) == len(wv) and len(gt) == len(wt), (what, len(gv), len(wv), len(gt), len(wt))
    assert gt.tobytes() == wt.tobytes(), what
    assert gv.tobytes() == wv.tobytes(), what


def _empty_engine(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    return pkg.SPHFluidGPU.from_particles(np.zeros(0, pkg.PARTICLE_DTYPE), sp)


def _cube_patterns():
    """All 256 inside patterns of one cube, each in its own cube of one lattice, separated by outside points."""
    f = np.zeros((3 * 4 + 1, 3 * 8 + 1, 3 * 8 + 1), F)
    for pat in range(256):
        a, b, c = pat % 8, (pat // 8) % 8, pat // 64
        for k in range(8):
            if (pat >> k) & 1:
                f[3 * c + 1 + ((k >> 2) & 1), 3 * b + 1 + ((k >> 1) & 1), 3 * a + 1 + (k & 1)] = 1.0
    return f


def test_volume_path_equals_the_restatement(pkg):
    rng = np.random.default_rng(5)
    eng = _empty_engine(pkg)
    cases = [("2x2x2", rng.random((2, 2, 2)).astype(F), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.5)]
    for shape in ((3, 5, 7), (9, 13, 11), (29, 17, 33)):
        cases.append((f"random {shape}", rng.random(shape).astype(F), (-3.25, -1.5, -7.0), (0.3, 0.7, 1.1), 0.5))
    q = rng.integers(0, 5, (17, 19, 23)).astype(F) * F(0.25)                 # many values exactly equal to iso
    cases.append(("values equal to iso", q, (-2.0, 0.5, -0.125), (0.25, 0.5, 0.375), 0.5))
    cases.append(("256 cube patterns", _cube_patterns(), (-1.0, -2.0, -3.0), (1.0, 1.0, 1.0), 0.5))
    n = (161, 163, 161)                                                        # 4 225 283 points >= 2^22: a smooth random field
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, k, dtype=np.float64) for k in n], indexing="ij")
    big = np.zeros(n, np.float64)
    for _ in range(6):
        c = rng.uniform(-0.7, 0.7, 3)
        big += np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / rng.uniform(0.02, 0.1))
    big = (big + 0.02 * rng.standard_normal(n)).astype(F)
    assert big.size >= 1 << 22
    cases.append(("4M smooth", big, (-10.5, 3.25, -0.75), (0.125, 0.0625, 0.09375), 0.6))
    for what, f, origin, spacing, iso in cases:
        want = _want(pkg, f, origin, spacing, iso)
        got = _volume_surface(pkg, eng, f, origin, spacing, iso)
        assert len(want[1]) > 0 or what == "2x2x2", what
        _assert_same(pkg, got, want, what)
    eng.close()


def test_nan_values(pkg):
    rng = np.random.default_rng(6)
    f = rng.random((15, 13, 11)).astype(F)
    f[rng.random(f.shape) < 0.1] = np.nan
    eng = _empty_engine(pkg)
    v, t = _volume_surface(pkg, eng, f, (0.5, -0.5, 1.0), (1.0, 0.5, 2.0), 0.5)
    eng.close()
    wv, wt = _want(pkg, f, (0.5, -0.5, 1.0), (1.0, 0.5, 2.0), 0.5)
    assert len(v) == len(wv) and t.tobytes() == wt.tobytes()
    assert len(t) > 0 and int(t.max()) < len(v)


def _states(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    yield "scene4096", np.load(os.path.join(G, "scene4096.npz"))["after_10"], sp
    z = np.load(os.path.join(G, "cylinder2000.npz"))
    sp = pkg.default_params(param_shapeType=2, param_boxHalf=(2.2, 1.6, 0.9), param_boxEulerDeg=(10.0, -25.0, 40.0),
                            param_boxCenter=(0.2, -0.1, 0.3), param_mass=float(z["mass"]))
    yield "cylinder2000", z["after"], sp
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    yield "settled_pool", fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))


def test_sampled_path_equals_volume_path_and_restatement(pkg):
    for name, rec, sp in _states(pkg):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        origin, spacing, dims = f.default_surface_lattice()
        for field in (pkg.SPH_FIELD_DENSITY, pkg.SPH_FIELD_FRACTION, pkg.SPH_FIELD_PRESSURE, pkg.SPH_FIELD_SPEED):
            vol = f.sample_lattice(origin, spacing, dims, field)
            pos = vol[vol > 0]
            iso = 0.5 if field == pkg.SPH_FIELD_FRACTION else float(np.quantile(pos, 0.4)) if len(pos) else 0.5
            got = f.surface(origin, spacing, dims, iso, field)
            assert len(got[1]) > 0, (name, field)
            _assert_same(pkg, got, _volume_surface(pkg, f, vol, origin, spacing, iso), (name, field, "volume"))
            _assert_same(pkg, got, _want(pkg, vol, origin, spacing, iso), (name, field, "restatement"))
        f.close()


def test_settled_pool_default_lattice(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    rec = fx["settled"]
    sp = pkg.default_params(param_mass=float(fx["mass"]))
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    origin, spacing, dims = f.default_surface_lattice()
    frac = f.sample_lattice(origin, spacing, dims, pkg.SPH_FIELD_FRACTION)
    v, t = f.surface()
    f.close()
    outer = np.concatenate([frac[0].ravel(), frac[-1].ravel(), frac[:, 0].ravel(), frac[:, -1].ravel(), frac[:, :, 0].ravel(), frac[:, :, -1].ravel()])
    assert (outer < 0.5).all()
    assert sr.closed_oriented(t)
    vol = sr.enclosed_volume(v["pos"], t)
    fluid = rec[rec["isGhost"] == 0]
    # The pool is settled in this engine's compressed regime (median density 7.5 rho0), so N mass / rho0 is not its volume; the
    # particles' own SPH volume sum(mass / rho_j) is (measured: 216.99 = 0.940 x 230.88, and 0.322 x N mass / rho0).
    want = float(np.sum(np.float64(sp.param_mass) / fluid["density"].astype(np.float64)))
    rest = len(fluid) * float(sp.param_mass) / float(sp.param_restDensity)
    print(f"settled pool: {len(v)} vertices, {len(t)} triangles, enclosed volume {vol:.4f} = {vol / want:.4f} x sum(mass / rho_j)"
          f" = {vol / rest:.4f} x N mass / rho0")
    assert abs(vol / want - 1.0) < 0.10


def test_extraction_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    h = sp.param_h

    def probe(f):
        f.surface()
        f.surface(f.ComputeGridExtents().gridMin, (h, h, h), (16, 16, 16), 500.0, pkg.SPH_FIELD_DENSITY)
    for aos, graph in ((1, 0), (0, 0), (1, 1), (0, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def test_repeats_and_scratch_reuse(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(3)
    state = f.download()
    a = f.surface()
    b = f.surface()
    _assert_same(pkg, a, b, "same call twice")
    g = f.ComputeGridExtents()
    h = sp.param_h
    small = ((g.gridMin[0] + 4 * h, g.gridMin[1], g.gridMin[2] + 4 * h), (h / 3, h / 3, h / 3), (11, 9, 13))
    rng = np.random.default_rng(9)
    vol_big = rng.random((40, 30, 50)).astype(F)
    vol_small = rng.random((3, 4, 5)).astype(F)
    seq = [("big", None), ("small", small), ("big", None)]
    got = [f.surface() if s is None else f.surface(*s) for _, s in seq]
    vgot = [_volume_surface(pkg, f, v, (0, 0, 0), (1, 1, 1), 0.5) for v in (vol_big, vol_small, vol_big)]
    f.close()
    for (what, s), gg, vv, vol in zip(seq, got, vgot, (vol_big, vol_small, vol_big)):
        fresh = pkg.SPHFluidGPU.from_particles(state, sp)
        _assert_same(pkg, gg, fresh.surface() if s is None else fresh.surface(*s), what)
        fresh.close()
        fresh = _empty_engine(pkg)
        _assert_same(pkg, vv, _volume_surface(pkg, fresh, vol, (0, 0, 0), (1, 1, 1), 0.5), "volume " + what)
        fresh.close()
    _assert_same(pkg, got[0], got[2], "big, small, big")


def test_refusals_and_edge_cases(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    vp, f3 = C.c_void_p, pkg.engine._f3
    s = pkg.SphSurface()
    ok_o, ok_s, ok_d = f3((0, 0, 0)), f3((0.5, 0.5, 0.5)), (C.c_int * 3)(4, 4, 4)
    dev = torch.zeros(64, dtype=torch.float32, device="cuda")
    # a z-slab engine
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    assert L.sph_extract_surface(slab._h, ok_o, ok_s, ok_d, pkg.SPH_FIELD_FRACTION, 0.5, C.byref(s)) == -3
    assert b"slab" in L.sph_last_error()
    assert L.sph_extract_surface_volume(slab._h, vp(dev.data_ptr()), ok_o, ok_s, ok_d, 0.5, C.byref(s)) == 0   # reads no particles
    slab.close()
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(2)                                                            # (the spawned records carry no density yet: fraction 0)
    h = f._h
    v4 = np.zeros(4, pkg.SURFACE_VERTEX_DTYPE)
    t4 = np.zeros((4, 3), np.uint32)
    assert L.sph_surface_download(h, v4.ctypes.data_as(vp), 4, t4.ctypes.data_as(vp), 4) == -3          # before any extract
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.surface()
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    bad = [((0, 4, 4), (1, 1, 1), 0.5, 1), ((4, 1, 4), (1, 1, 1), 0.5, 1), ((4, 4, -2), (1, 1, 1), 0.5, 1),
           ((65536, 65536, 2), (1, 1, 1), 0.5, 1), ((1 << 16, 1 << 10, 1 << 5), (1, 1, 1), 0.5, 1),
           ((4, 4, 4), (float("nan"), 1, 1), 0.5, 1), ((4, 4, 4), (1, 0, 1), 0.5, 1), ((4, 4, 4), (1, 1, -1), 0.5, 1),
           ((4, 4, 4), (1, float("inf"), 1), 0.5, 1), ((4, 4, 4), (1, 1, 1), float("nan"), 1), ((4, 4, 4), (1, 1, 1), float("inf"), 1),
           ((4, 4, 4), (1, 1, 1), 0.5, pkg.SPH_FIELD_ALL), ((4, 4, 4), (1, 1, 1), 0.5, 5), ((4, 4, 4), (1, 1, 1), 0.5, -1)]
    for dims, spacing, iso, field in bad:
        d = (C.c_int * 3)(*dims)
        assert L.sph_extract_surface(h, ok_o, f3(spacing), d, field, iso, C.byref(s)) == -1, (dims, spacing, iso, field)
        if field == 1:
            assert L.sph_extract_surface_volume(h, vp(dev.data_ptr()), ok_o, f3(spacing), d, iso, C.byref(s)) == -1, (dims, spacing, iso)
    assert L.sph_extract_surface(h, None, ok_s, ok_d, 1, 0.5, C.byref(s)) == -1
    assert L.sph_extract_surface(h, ok_o, None, ok_d, 1, 0.5, C.byref(s)) == -1
    assert L.sph_extract_surface(h, ok_o, ok_s, None, 1, 0.5, C.byref(s)) == -1
    assert L.sph_extract_surface(h, ok_o, ok_s, ok_d, 1, 0.5, None) == -1
    assert L.sph_extract_surface_volume(h, None, ok_o, ok_s, ok_d, 0.5, C.byref(s)) == -1
    # short capacities: SPH_ERR_CAPACITY and nothing written
    v, t = f.surface()
    assert len(v) > 4 and len(t) > 4
    vb = np.zeros(len(v), pkg.SURFACE_VERTEX_DTYPE)
    vb.view(np.uint8)[:] = 0xAB
    tb = np.full((len(t), 3), 0xABABABAB, np.uint32)
    assert L.sph_surface_download(h, vb.ctypes.data_as(vp), len(v) - 1, tb.ctypes.data_as(vp), len(t)) == -4
    assert L.sph_surface_download(h, vb.ctypes.data_as(vp), len(v), tb.ctypes.data_as(vp), len(t) - 1) == -4
    assert (vb.view(np.uint8) == 0xAB).all() and (tb == 0xABABABAB).all()
    assert L.sph_surface_download(h, vb.ctypes.data_as(vp), len(v), tb.ctypes.data_as(vp), len(t)) == 0
    assert vb.tobytes() == v.tobytes() and tb.tobytes() == t.tobytes()
    # the borrowed device arrays hold the same bytes
    surf = f.extract_surface(*f.default_surface_lattice())
    assert (surf.numVertices, surf.numTriangles) == (len(v), len(t))
    hv = np.zeros(len(v), pkg.SURFACE_VERTEX_DTYPE)
    ht = np.zeros((len(t), 3), np.uint32)
    hip = C.CDLL("libamdhip64.so.7")                                      # (already loaded by the engine)
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    f.sync()
    assert hip.hipMemcpy(hv.ctypes.data_as(vp), vp(surf.vertices), len(v) * 24, 2) == 0              # hipMemcpyDeviceToHost
    assert hip.hipMemcpy(ht.ctypes.data_as(vp), vp(surf.triangles), len(t) * 12, 2) == 0
    assert hv.tobytes() == v.tobytes() and ht.tobytes() == t.tobytes()
    # a failed extract leaves no surface
    assert L.sph_extract_surface(h, ok_o, f3((0, 1, 1)), ok_d, 1, 0.5, C.byref(s)) == -1
    assert L.sph_surface_download(h, vb.ctypes.data_as(vp), len(v), tb.ctypes.data_as(vp), len(t)) == -3
    # an empty surface: counts 0
    v0, t0 = f.surface(iso=1e9)
    assert len(v0) == 0 and len(t0) == 0
    assert L.sph_surface_download(h, None, 0, None, 0) == 0
    f.ResetSimulation(seed=4)
    assert L.sph_surface_download(h, None, 0, None, 0) == -3                                              # reset ends the surface
    f.close()
    e = _empty_engine(pkg)
    v, t = e.surface()
    assert len(v) == 0 and len(t) == 0
    e.close()


def _parse_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert "format binary_little_endian 1.0" in lines
    assert len(body) == 24 * nv + 13 * nf
    v = np.frombuffer(body[: 24 * nv], np.float32).reshape(nv, 6)
    faces = np.frombuffer(body[24 * nv:], np.dtype([("n", "u1"), ("idx", "<u4", (3,))]))
    assert (faces["n"] == 3).all()
    return v, faces["idx"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_surface_mesh_example(pkg, tmp_path):
    out = tmp_path / "frames"
    out.mkdir()
    res = run_example(build_example(pkg, "surface_mesh", tmp_path), [out, "3"], timeout=300)
    assert res.returncode == 0 and "surface_mesh OK" in res.stdout
    frames = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(frames) == 3
    for k, ln in enumerate(frames):
        v, t = _parse_ply(out / f"frame_{k:04d}.ply")
        nv, nt = (int(tok.split("=")[1]) for tok in ln.split()[2:])
        assert (len(v), len(t)) == (nv, nt) and nt > 1000
        assert sr.closed_oriented(t) and int(t.max()) < len(v)
        assert np.isfinite(v).all()


def test_full_size_scene(pkg):
    """BASELINE.json configs[2] (4 194 304 particles, 128^3 cells), default lattice: a closed, oriented mesh."""
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    sp = pkg.default_params(**syn.params_fields(cfg))
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchCompute()                                                       # (the spawned records carry no density yet: fraction 0)
    origin, spacing, dims = f.default_surface_lattice()
    v, t = f.surface()
    f.close()
    print(f"configs[2]: lattice {dims}, {len(v)} vertices, {len(t)} triangles")
    assert len(t) > 100000
    assert int(t.max()) < len(v) and len(np.unique(t)) == len(v)
    assert sr.closed_oriented(t)
