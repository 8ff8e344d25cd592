"""Field sampling on the GPU (include/sph_abi.h "field sampling"): identity with the SPH pass, the float64 brute force, lattice = points,
mass, no perturbation of the simulation, freshness, refusals, the wave gauge and the C++ example.

Tolerances against the float64 brute force (tests/sample_ref.brute), derived from the fp32 arithmetic: a neighbour's r^2 carries the
rounding of x - x_j (2^-24 relative per axis) and of dot3 (two roundings), i.e. |dr^2| <= ~3e-7 h^2, so t^3 is off by at most
3 t^2 |dt| <= ~1e-6 h^6 per neighbour; the fp32 sum adds 2^-24 relative per term.  Hence
  |density - ref| <= 1e-5 |ref| + 2e-6 (count + 1) mp6 h^6,   the same for fraction with mp6 h^6 max(1/rho_j),
which sample_ref's emulation of the arithmetic meets on CPU (tests/test_sample_cpu.py::test_tolerances_hold_for_the_fp32_arithmetic).
count is exact except for pairs with |r^2 - h^2| <= 1e-5 h^2 (excluded).  The Shepard quotients (vel, pressure) are compared where the
reference's fraction is >= 0.05: both sums are then within ~2.5e-3 relative of float64, so the quotient within 5e-3 max |v_j|."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT, assert_records_equal, small_scene, to_oracle_params
import sample_ref
from support import build_example, identity_states, run_example, undisturbed_run

pytestmark = pytest.mark.gpu

G = os.path.join(ROOT, "tests", "golden")
F = np.float32


def test_density_at_the_particles_is_the_next_substeps_density(pkg, oracle):
    for name, rec, sp in identity_states(pkg):
        op = to_oracle_params(oracle, sp)
        fluid = rec["isGhost"] == 0
        want_oracle = oracle.substep(rec, op)["density"]
        b = oracle.build_grid(rec, op)
        _, _, cnt = sample_ref.emulate(rec, rec["pos"], sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"])
        half = F(0.5) * F(sp.param_restDensity)
        for kern in (1, 2, 3):
            f = pkg.SPHFluidGPU.from_particles(rec, sp)
            f.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, kern)
            s = f.sample(rec["pos"])
            f.DispatchCompute()
            got = f.download()["density"]
            f.close()
            d = np.maximum(s["density"], half)
            assert np.array_equal(d[fluid].view(np.uint32), got[fluid].view(np.uint32)), (name, kern)
            assert np.array_equal(d[fluid].view(np.uint32), want_oracle[fluid].view(np.uint32)), (name, kern)
            assert np.array_equal(s["count"], cnt), (name, kern)


def _probes(g, h, rng, n_random=12000):
    lo = np.array(g.gridMin, F)
    cs = F(g.cellSize)
    dims = np.array(g.dims)
    hi = lo + cs * dims.astype(F)
    parts = [(lo + (hi - lo) * rng.random((n_random, 3))).astype(F)]
    faces = (lo + (hi - lo) * rng.random((2500, 3))).astype(F)         # exactly on cell faces along one axis
    ax = rng.integers(0, 3, len(faces))
    k = rng.integers(0, dims.max() + 1, len(faces))
    faces[np.arange(len(faces)), ax] = (lo[ax] + k.astype(F) * cs).astype(F)
    parts.append(faces)
    parts.append((lo + cs * rng.integers(0, dims + 1, (1000, 3)).astype(F)).astype(F))     # cell corners
    top = lo.copy()
    top[1] = hi[1] - F(1.5) * cs
    parts.append((top + (hi - top) * rng.random((1500, 3))).astype(F))                    # high up: mostly empty cells
    out = (lo - 3 * cs + (hi - lo + 6 * cs) * rng.random((2000, 3))).astype(F)            # around and outside the grid
    parts.append(out)
    nf = (lo + (hi - lo) * rng.random((1000, 3))).astype(F)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    nf[np.arange(len(nf)), rng.integers(0, 3, len(nf))] = bad[rng.integers(0, 3, len(nf))]
    parts.append(nf)
    return np.concatenate(parts)


def _check_against_brute(pkg, s, rec, pts, sp, what):
    h = float(sp.param_h)
    bf = sample_ref.brute(rec, pts, h, sp.param_mass)
    mp6h6 = float(F(sp.param_mass)) * 315.0 / (64.0 * np.pi * h ** 3)
    rho = rec["density"][rec["density"] > 0]
    inv_max = float((1.0 / rho).max()) if len(rho) else 0.0
    dt = 1e-5 * np.abs(bf["density"]) + 2e-6 * (bf["count"] + 1) * mp6h6
    ft = 1e-5 * np.abs(bf["fraction"]) + 2e-6 * (bf["count"] + 1) * mp6h6 * inv_max
    assert np.all(np.abs(s["density"] - bf["density"]) <= dt), what
    assert np.all(np.abs(s["fraction"] - bf["fraction"]) <= ft), what
    sure = bf["edge"] == 0
    assert np.array_equal(s["count"][sure].astype(np.int64), bf["count"][sure]), what
    assert np.all(np.abs(s["count"].astype(np.int64) - bf["count"]) <= bf["edge"]), what
    core = bf["fraction"] >= 0.05
    vmax = float(np.abs(rec["vel"][:, :3]).max()) if len(rec) else 0.0
    pmax = float(np.abs(rec["pressure"]).max()) if len(rec) else 0.0
    assert np.all(np.abs(s["vel"][core] - bf["vel"][core]) <= 5e-3 * vmax + 1e-6), what
    assert np.all(np.abs(s["pressure"][core] - bf["pressure"][core]) <= 5e-3 * pmax + 1e-6), what
    fin = np.isfinite(pts).all(axis=1)
    assert not s[~fin].tobytes().strip(b"\0"), what                              # non-finite probes: all-zero records
    return bf


def test_fields_against_the_float64_brute_force(pkg):
    rng = np.random.default_rng(11)
    rec0, sp0 = small_scene(pkg, n=4096, grid=16, seed=7)
    rec1, sp1 = small_scene(pkg, n=4096, grid=16, seed=3)
    for name, rec, sp, steps in (("scene4096", np.load(os.path.join(G, "scene4096.npz"))["after_10"], sp0, 0), ("small_scene", rec1, sp1, 3)):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        if steps:
            f.DispatchN(steps)
        state = f.download()
        g = f.ComputeGridExtents()
        pts = _probes(g, sp.param_h, rng)
        s = f.sample(pts)
        f.close()
        bf = _check_against_brute(pkg, s, state, pts, sp, name)
        assert (bf["count"] == 0).sum() > 500 and (bf["count"] >= 3).sum() > 2000      # the probes reach empty space and the fluid


def _lattice_points(origin, spacing, dims):
    axes = [F(origin[a]) + np.arange(dims[a], dtype=F) * F(spacing[a]) for a in range(3)]
    Z, Y, X = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1).astype(F)


def _lattice_equals_points(pkg, f, origin, spacing, dims, what):
    pts = _lattice_points(origin, spacing, dims)
    want = f.sample(pts)
    allf = f.sample_lattice(origin, spacing, dims, pkg.SPH_FIELD_ALL)
    assert allf.shape == (dims[2], dims[1], dims[0])
    assert allf.reshape(-1).tobytes() == want.tobytes(), what
    v = want["vel"]
    speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)
    for field, ref in ((pkg.SPH_FIELD_DENSITY, want["density"]), (pkg.SPH_FIELD_FRACTION, want["fraction"]),
                       (pkg.SPH_FIELD_PRESSURE, want["pressure"]), (pkg.SPH_FIELD_SPEED, speed)):
        got = f.sample_lattice(origin, spacing, dims, field)
        assert got.dtype == F and got.reshape(-1).tobytes() == np.ascontiguousarray(ref, F).tobytes(), (what, field)
    return want


def test_lattice_equals_points(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(3)
    g = f.ComputeGridExtents()
    h = sp.param_h
    origin = (g.gridMin[0] - 0.3 * h, g.gridMin[1] + 0.17 * h, g.gridMin[2] - 1.1 * h)
    dims = (37, 29, 21)
    want = _lattice_equals_points(pkg, f, origin, (h / 2, h / 2, h / 2), dims, "h/2")
    assert (want["count"] > 0).sum() > 1000
    _lattice_equals_points(pkg, f, (g.gridMin[0], g.gridMin[1], g.gridMin[2]), (3.1 * h, 0.7 * h, 1.9 * h), (9, 17, 5), "coarse")
    f.close()
    # every particle in one cell: no brick's rows fit in LDS (the global-memory path)
    one = rec.copy()
    c = np.array(g.gridMin, F) + F(g.cellSize) * (np.array(g.dims) // 2).astype(F)
    rng = np.random.default_rng(5)
    one["pos"][:, :3] = c + F(g.cellSize) * (F(0.05) + F(0.9) * rng.random((len(one), 3)).astype(F))
    f = pkg.SPHFluidGPU.from_particles(one, sp)
    cnt, _ = f.download_grid()
    assert cnt.max() == len(one)
    want = _lattice_equals_points(pkg, f, (c[0] - 2 * h, c[1] - 2 * h, c[2] - 2 * h), (h / 4, h / 4, h / 4), (20, 20, 20), "one cell")
    assert want["count"].max() == len(one)
    f.close()


def test_mass_of_the_density_field(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    h = sp.param_h
    pos = rec["pos"][:, :3]
    s = F(h / 2)
    origin = (pos.min(axis=0) - F(1.25 * h)).astype(F)
    dims = tuple(int(x) for x in np.ceil((pos.max(axis=0) + F(1.25 * h) - origin) / s).astype(int) + 1)
    dens = f.sample_lattice(origin, (s, s, s), dims, pkg.SPH_FIELD_DENSITY)
    f.close()
    total = float(dens.astype(np.float64).sum()) * float(s) ** 3
    assert abs(total / (len(rec) * float(sp.param_mass)) - 1.0) < 0.005


def test_sampling_does_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    h = sp.param_h
    pts = rec["pos"][::7, :3]

    def probe(f):
        g = f.ComputeGridExtents()
        f.sample(pts)
        f.sample_lattice(g.gridMin, (h / 2, h / 2, h / 2), (24, 24, 24), pkg.SPH_FIELD_ALL)
        f.sample_lattice(g.gridMin, (h, h, h), (16, 16, 16), pkg.SPH_FIELD_DENSITY)
    for aos, graph in ((1, 0), (0, 0), (1, 1), (0, 1)):
        a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
        b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
        assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
        assert_records_equal(a, b, f"aos {aos} graph {graph}")
        if graph:
            assert la > 0 and lb > 0


def test_samples_are_fresh(pkg):
    rng = np.random.default_rng(3)
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)

    def check(what):
        state = f.download()
        g = f.ComputeGridExtents()
        pts = _probes(g, sp.param_h, rng, n_random=3000)[:6000]
        pts = pts[np.isfinite(pts).all(axis=1)]
        _check_against_brute(pkg, f.sample(pts), state, pts, sp, what)
    check("before the first dispatch")
    f.DispatchN(3)
    check("after dispatches")
    f.ApplyWaveImpulse(2.5, 3.0, 0.25, (0.0, 1.0, 0.0))
    check("after ApplyWaveImpulse")
    moved = f.download()
    moved["pos"][:, 1] += F(0.37 * sp.param_h)
    f.upload(moved)
    check("after upload")
    f.param_boxCenter = (0.2 * sp.param_h, 0.0, -0.3 * sp.param_h)
    check("after a box move")
    f.numParticles = 3000
    f.ResetSimulation(seed=9)
    check("after ResetSimulation")
    f.close()


def test_refusals_and_edge_cases(pkg):
    import torch
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    out = np.zeros(4, pkg.SAMPLE_DTYPE)
    pts = np.zeros((4, 4), F)
    vp = C.c_void_p
    # a z-slab engine
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    assert L.sph_sample_points(slab._h, pts.ctypes.data_as(vp), 4, out.ctypes.data_as(vp)) == -3
    assert b"slab" in L.sph_last_error()
    dev = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert L.sph_sample_lattice(slab._h, pkg.engine._f3((0, 0, 0)), pkg.engine._f3((1, 1, 1)), (C.c_int * 3)(2, 2, 2), 0, vp(dev.data_ptr())) == -3
    slab.close()
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.sample(pts[:, :3])
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    h = f._h
    assert L.sph_sample_points(h, None, 4, out.ctypes.data_as(vp)) == -1
    assert L.sph_sample_points(h, pts.ctypes.data_as(vp), 4, None) == -1
    assert L.sph_sample_points_device(h, None, 4, vp(dev.data_ptr())) == -1
    assert L.sph_sample_points(None, pts.ctypes.data_as(vp), 4, out.ctypes.data_as(vp)) == -1
    f3 = pkg.engine._f3
    for dims, spacing, field in (((0, 2, 2), (1, 1, 1), 0), ((2, -1, 2), (1, 1, 1), 0), ((65536, 65536, 1), (1, 1, 1), 0),
                                 ((1 << 16, 1 << 10, 1 << 5), (1, 1, 1), 0),
                                 ((2, 2, 2), (float("nan"), 1, 1), 0), ((2, 2, 2), (1, 0, 1), 0), ((2, 2, 2), (1, 1, -1), 0),
                                 ((2, 2, 2), (1, float("inf"), 1), 0), ((2, 2, 2), (1, 1, 1), 5), ((2, 2, 2), (1, 1, 1), -1)):
        assert L.sph_sample_lattice(h, f3((0, 0, 0)), f3(spacing), (C.c_int * 3)(*dims), field, vp(dev.data_ptr())) == -1, (dims, spacing, field)
    assert L.sph_sample_lattice(h, None, f3((1, 1, 1)), (C.c_int * 3)(2, 2, 2), 0, vp(dev.data_ptr())) == -1
    assert L.sph_sample_lattice(h, f3((0, 0, 0)), f3((1, 1, 1)), (C.c_int * 3)(2, 2, 2), 0, None) == -1
    # 2^31 - 1 points exactly is accepted by the checks (not launched here: 8 GiB of output); m = 0 is valid
    assert len(f.sample(np.zeros((0, 3), F))) == 0
    assert L.sph_sample_points_device(h, None, 0, None) == 0
    # the device variant with torch tensors
    state = f.download()
    p4 = torch.zeros((len(state), 4), dtype=torch.float32, device="cuda")
    p4[:, :3] = torch.from_numpy(state["pos"][:, :3].copy()).cuda()
    o = torch.zeros((len(state), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                      # the fills run on torch's stream, the kernel on the engine's own
    f.sample_device(p4.data_ptr(), len(state), o.data_ptr())
    f.sync()
    assert o.cpu().numpy().tobytes() == f.sample(state["pos"][:, :3]).tobytes()
    f.close()
    # N = 0: every result is zero
    e = pkg.SPHFluidGPU.from_particles(np.zeros(0, pkg.PARTICLE_DTYPE), sp)
    s = e.sample(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], F))
    assert len(s) == 2 and not s.tobytes().strip(b"\0")
    lat = e.sample_lattice((0, 0, 0), (0.5, 0.5, 0.5), (9, 3, 5), pkg.SPH_FIELD_ALL)
    assert lat.shape == (5, 3, 9) and not lat.tobytes().strip(b"\0")
    e.close()


def test_water_level_on_the_settled_pool(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    rec = fx["settled"]
    sp = pkg.default_params(param_mass=float(fx["mass"]))
    h = sp.param_h
    pos = rec["pos"][:, :3]
    cols = np.array([[0.0, 0.0], [2.0, -1.5], [-3.0, 2.5], [4.5, 4.0]], F)
    y_lo, y_hi, dy = float(pos[:, 1].min()) - h, float(pos[:, 1].max()) + 2 * h, h / 8
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    lv = f.water_level(cols, y_lo, y_hi, dy)
    f.close()
    ys, pts = sample_ref.gauge_columns(None, cols, y_lo, y_hi, dy)
    bf = sample_ref.brute(rec, pts.reshape(-1, 3), h, float(fx["mass"]))
    want = pkg.gauge_levels(bf["fraction"].reshape(len(cols), len(ys)), ys)
    assert np.all(np.isfinite(lv))
    # the fraction differs from float64 by <= ~1e-4 near the surface, where it changes by ~0.3 per sample (h / 8): far below 0.01 h
    assert np.all(np.abs(lv - want) < 0.01 * h), (lv, want)
    for c, (x, z) in enumerate(cols):
        near = (np.abs(pos[:, 0] - x) < 0.5 * h) & (np.abs(pos[:, 2] - z) < 0.5 * h)
        assert abs(lv[c] - float(pos[near, 1].max())) < 0.5 * h


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_wave_gauge_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "wave_gauge", tmp_path), ["50000", "12"], timeout=300)
    assert res.returncode == 0 and "wave_gauge OK" in res.stdout
    frames = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(frames) == 12
    for ln in frames:
        vals = [float(tok.split("=")[1]) for tok in ln.split()[2:]]
        assert len(vals) == 3 and all(np.isfinite(vals)), ln
