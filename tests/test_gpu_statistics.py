"""State statistics on the GPU (include/sph_abi.h "statistics"): equal bits with the numpy restatement
(tests/stats_ref.py), a pure function of the state, agreement with the download, no perturbation of the simulation, freshness,
the watchdog counts, refusals, the device variant and the C++ example.

Bound for the fp64 sums against exact arithmetic (math.fsum of the same terms): gamma_d * fsum(|terms|) with
gamma_d = d u / (1 - d u), u = 2^-53 and d = the tree's depth (11 + log2 of the padded tile count) plus the roundings inside one
term (stats_ref.TERM_ROUNDINGS).  Derived from the standard error bound of pairwise summation, not measured."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT, assert_records_equal, small_scene
import stats_ref
from support import build_example, run_example

pytestmark = pytest.mark.gpu

G = os.path.join(ROOT, "tests", "golden")
F = np.float32
SPECS = [(stats_ref.DENSITY, 256, 0.0, 8000.0), (stats_ref.SPEED, 1024, 0.0, 40.0), (stats_ref.POS_Y, 100, -2.5, 2.5), (stats_ref.FOAM, 1, 0.0, 1.0)]


def _reference(pkg, f, specs=SPECS):
    """The restatement on what the engine itself reports: its download, its members, the grid they imply, its cells."""
    rec = f.download()
    _, cells = f.download_grid()
    return stats_ref.statistics(rec, f.params, f.ComputeGridExtents(), cells, specs), rec


def _assert_equal_bits(pkg, f, what, specs=SPECS):
    ref, rec = _reference(pkg, f, specs)
    got = f.statistics(specs)
    want = stats_ref.pack(ref, pkg.SphStatistics)
    gb, wb = bytes(got.s), bytes(want)
    for name, _ in pkg.SphStatistics._fields_:
        fld = getattr(pkg.SphStatistics, name)
        a, b = gb[fld.offset:fld.offset + fld.size], wb[fld.offset:fld.offset + fld.size]
        if a != b:
            kind = "<f8" if name.startswith("sum") else "<u4"
            raise AssertionError(f"{what}: SphStatistics.{name} differs: {np.frombuffer(a, kind)} vs {np.frombuffer(b, kind)}")
    assert gb == wb, what
    assert len(got.histograms) == len(specs)
    for k, (h, w) in enumerate(zip(got.histograms, ref["histograms"])):
        assert np.array_equal(h, w), (what, "histogram", k)
        assert int(h.sum()) == ref["numCounted"], (what, "histogram", k)
    assert got.tobytes() == stats_ref.to_bytes(ref, pkg.SphStatistics), what
    return got, ref, rec


def _river_scene(pkg, n=6000, seed=5):
    sp = pkg.default_params()
    river, heights = pkg.generate_river_terrain(sp, seed)
    river.riverMode = 1
    P, mass = pkg.spawn_river_particles(sp, river, heights, n, 11)
    sp.param_mass = mass
    return P, sp, river, heights


def _ghost_scene(pkg):
    rec, sp = small_scene(pkg, n=6000, grid=20, seed=35)
    rng = np.random.default_rng(9)
    P = rec.copy()
    P["vel"][:, :3] += rng.normal(0, 5, (len(P), 3)).astype(F)
    P["padA"] = rng.random(len(P)).astype(F)
    P["isGhost"][2000:2040] = 1
    P["isActive"][2000:2020] = 1
    P["isGhost"][2040:2060] = 3
    P["isActive"][100:200] = 1                                              # isActive does not enter the definition of fluid
    return P, sp


def _small_states(pkg):
    z = np.load(os.path.join(G, "scene4096.npz"))
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    for key in ("initial", "after_1", "after_100"):
        yield "scene4096 " + key, z[key], sp
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    yield "settled_pool", fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    c = np.load(os.path.join(G, "cylinder2000.npz"))
    sp = pkg.default_params(param_shapeType=2, param_boxHalf=(2.2, 1.6, 0.9), param_boxEulerDeg=(10.0, -25.0, 40.0),
                            param_boxCenter=(0.2, -0.1, 0.3), param_mass=float(c["mass"]))
    yield "cylinder2000", c["after"], sp
    P, sp = _ghost_scene(pkg)
    yield "ghosts", P, sp


# ---- 1. equal bits ------------------------------------------------------------------------------------------------------------------
def test_equal_bits_with_the_restatement_small_states(pkg):
    for name, rec, sp in _small_states(pkg):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        got, ref, _ = _assert_equal_bits(pkg, f, name)
        f.DispatchN(3)
        _assert_equal_bits(pkg, f, name + " + 3 substeps")
        f.close()
        if name == "settled_pool":
            assert set(rec["isActive"]) == {0} and got.numFluid == got.numCounted == len(rec)      # fluid does not depend on isActive
        if name == "ghosts":
            assert (got.numActiveGhosts, got.numInactiveGhosts, got.numOther) == (20, 20, 20) and got.numFluid == len(rec) - 60


def test_equal_bits_river_scene(pkg):
    P, sp, river, heights = _river_scene(pkg)
    f = pkg.SPHFluidGPU.from_particles(P, sp)
    f.set_river(river, heights)
    _assert_equal_bits(pkg, f, "river initial")
    f.DispatchN(20)
    _assert_equal_bits(pkg, f, "river after 20")
    f.close()


def test_equal_bits_config3_four_million(pkg):
    """BASELINE.json configs[2]: 4 194 304 particles, after 1 and after 60 substeps."""
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    assert len(rec) == 4194304
    sp = pkg.default_params(**syn.params_fields(cfg))
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    del rec
    rho0 = float(sp.param_restDensity)
    specs = [(stats_ref.DENSITY, 256, 0.0, 4 * rho0), (stats_ref.PRESSURE, 256, 0.0, 2.0e6), (stats_ref.SPEED, 256, 0.0, 120.0),
             (stats_ref.POS_Y, 256, -float(sp.param_boxHalf[1]), float(sp.param_boxHalf[1]))]
    f.DispatchCompute()
    got, _, _ = _assert_equal_bits(pkg, f, "config 3 after 1", specs)
    assert got.numCounted == 4194304 and got.ok
    f.DispatchN(59)
    _assert_equal_bits(pkg, f, "config 3 after 60", specs)
    f.close()


# ---- 2. pure function of the state --------------------------------------------------------------------------------------------------------
def test_pure_function_of_the_state(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    rec0, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    want = None
    for aos in (1, 0):
        for kern in (1, 2, 3):
            for graph in (0, 1):
                f = pkg.SPHFluidGPU.from_particles(rec0, sp)
                f.set_option(pkg.SPH_OPT_AOS_MODE, aos)
                f.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, kern)
                f.set_option(pkg.SPH_OPT_GRAPH, graph)
                for _ in range(4):
                    f.DispatchN(4)                                          # (with SPH_OPT_GRAPH: eager, eager, capture + replay, replay)
                a = f.statistics(SPECS).tobytes()
                b = f.statistics(SPECS).tobytes()                           # twice in a row
                f.sample(rec0["pos"][:100])
                f.surface()
                c = f.statistics(SPECS).tobytes()                           # after sample() / surface()
                assert a == b == c, (aos, kern, graph)
                if want is None:
                    want = a
                    g = pkg.SPHFluidGPU.from_particles(f.download(), sp)    # a second engine created from the first one's download
                    assert g.statistics(SPECS).tobytes() == want
                    g.close()
                assert a == want, (aos, kern, graph)
                f.close()


# ---- 3. against the download ------------------------------------------------------------------------------------------------------------
def test_against_numpy_on_the_download(pkg):
    for name, rec0, sp in _small_states(pkg):
        f = pkg.SPHFluidGPU.from_particles(rec0, sp)
        f.DispatchN(2)
        s = f.statistics()
        rec = f.download()
        f.close()
        fl = rec["isGhost"] == 0
        ids = np.nonzero(fl)[0]
        c = rec[fl]
        assert s.numRecords == len(rec) and s.numFluid == s.numCounted == int(fl.sum()) and s.numNonFinite == 0
        for a in range(3):
            assert s.minPos[a].value == c["pos"][:, a].min() and s.minPos[a].id == ids[np.argmin(c["pos"][:, a])], name
            assert s.maxPos[a].value == c["pos"][:, a].max() and s.maxPos[a].id == ids[np.argmax(c["pos"][:, a])], name
        assert s.minDensity.value == c["density"].min() and s.minDensity.id == ids[np.argmin(c["density"])], name
        assert s.maxDensity.value == c["density"].max() and s.maxDensity.id == ids[np.argmax(c["density"])], name
        assert s.minPressure.value == c["pressure"].min() and s.maxPressure.value == c["pressure"].max(), name
        assert s.maxFoam.value == c["padA"].max() and s.maxFoam.id == ids[np.argmax(c["padA"])], name
        v = c["vel"]
        s2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        assert s.maxSpeed2.value == s2.max() and s.maxSpeed2.id == ids[np.argmax(s2)] and s.maxSpeed == np.sqrt(s2.max()), name
        t = stats_ref.terms(rec, fl, sp.param_boxCenter)
        got = dict(zip(stats_ref.SUM_NAMES, list(s.sumPos) + list(s.sumVel) + [s.sumSpeed2, s.sumDensity, s.sumDensity2, s.sumPressure, s.sumFoam,
                                                                                 s.sumInvDensity] + list(s.sumAngular)))
        u = 2.0 ** -53
        for k in stats_ref.SUM_NAMES:
            d = stats_ref.tree_depth(len(rec)) + stats_ref.TERM_ROUNDINGS[k]
            bound = d * u / (1 - d * u) * math.fsum(np.abs(t[k]))
            err = abs(got[k] - math.fsum(t[k]))
            print(f"{name} sum {k}: error {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, k, err, bound)
        assert s.kinetic_energy == 0.5 * float(sp.param_mass) * s.sumSpeed2 and s.cfl == s.maxSpeed * float(sp.param_timeStep) / float(sp.param_h)


# ---- 4. no perturbation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_statistics_do_not_perturb_the_simulation(pkg, graph):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    a = pkg.SPHFluidGPU.from_particles(rec, sp)
    b = pkg.SPHFluidGPU.from_particles(rec, sp)
    for f in (a, b):
        f.set_option(pkg.SPH_OPT_GRAPH, graph)
    for step in range(12):
        a.DispatchN(4 if graph else 1)
        b.DispatchN(4 if graph else 1)
        b.statistics(SPECS)
    assert_records_equal(b.download(), a.download(), f"statistics between substeps (graph {graph})")
    a.close()
    b.close()


# ---- 5. freshness -----------------------------------------------------------------------------------------------------------------------
def test_result_follows_the_state_and_the_members(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    s0, _, _ = _assert_equal_bits(pkg, f, "initial")
    f.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
    s1, _, _ = _assert_equal_bits(pkg, f, "after an impulse")
    assert s1.sumSpeed2 != s0.sumSpeed2
    other = rec.copy()
    other["pos"][:, 0] += F(0.125)
    f.upload(other)
    s2, _, _ = _assert_equal_bits(pkg, f, "after upload")
    assert s2.sumPos[0] != s1.sumPos[0]
    f.param_h = 0.35                                                        # a member edit that changes the grid
    s3, _, _ = _assert_equal_bits(pkg, f, "after param_h edit")
    assert list(s3.occupancy) != list(s2.occupancy)
    f.param_boxHalf = (1.0, 1.0, 1.0)                                       # a smaller grid: particles now lie outside it
    s4, _, _ = _assert_equal_bits(pkg, f, "after param_boxHalf edit")
    assert s4.numEscaped > s3.numEscaped and s4.firstEscapedId != 0xFFFFFFFF
    f.close()
    g = pkg.SPHFluidGPU(5000, seed=3)
    g.DispatchN(3)
    _assert_equal_bits(pkg, g, "spawned + 3")
    g.ResetSimulation()
    r, _, _ = _assert_equal_bits(pkg, g, "after ResetSimulation")
    g.close()
    fresh = pkg.SPHFluidGPU(5000, seed=3)
    assert r.tobytes() == fresh.statistics(SPECS).tobytes()
    fresh.close()


# ---- 6. watchdog ----------------------------------------------------------------------------------------------------------------------
def test_watchdog_counts_non_finite_and_escaped_records(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    P = rec.copy()
    a, b, c = 700, 1900, 3000
    P["vel"][a, 1] = np.nan
    P["density"][b] = np.inf
    P["pos"][c, :3] = (50.0, 60.0, -70.0)
    f = pkg.SPHFluidGPU.from_particles(P, sp)
    got, ref, _ = _assert_equal_bits(pkg, f, "poisoned upload")
    f.close()
    assert got.numNonFinite == 2 and got.firstNonFiniteId == a
    assert got.numEscaped >= 1 and got.firstEscapedId == c and not got.ok
    assert got.numCounted == len(P) - 2


def test_empty_counted_set(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    P = rec[:300].copy()
    P["isGhost"] = 1
    f = pkg.SPHFluidGPU.from_particles(P, sp)
    got, _, _ = _assert_equal_bits(pkg, f, "ghosts only")
    f.close()
    assert got.numCounted == 0 and got.minDensity.value == np.inf and got.maxDensity.value == -np.inf and got.maxSpeed2.id == 0xFFFFFFFF
    assert got.maxSpeed == 0.0 and got.sumSpeed2 == 0.0 and got.occupiedCells > 0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    """The documented code and a message for every refused call, and an engine that still works afterwards.  (That a refused call
    allocates nothing follows from the order in sph_statistics: refusal and spec checks come before the first allocation; the
    C-ABI offers no way to observe an engine's allocations, so it is not asserted here.)"""
    from importlib import import_module
    L = pkg.load_library()
    vp = C.c_void_p
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    out = pkg.SphStatistics()
    hist = np.zeros(8192, np.uint64)
    hp = hist.ctypes.data_as(vp)

    def spec(*rows):
        arr = (pkg.SphHistogramSpec * len(rows))()
        for i, r in enumerate(rows):
            arr[i] = pkg.SphHistogramSpec(*r)
        return arr
    ok = spec((0, 16, 0.0, 1.0))
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    assert L.sph_statistics(slab._h, C.byref(out), ok, 1, hp) == -3
    assert b"slab" in L.sph_last_error()
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    assert L.sph_statistics(f._h, C.byref(out), ok, 1, hp) == -3
    assert b"SPH_OPT_GRID_BUILD" in L.sph_last_error()
    with pytest.raises(pkg.SphError, match="-3"):
        f.statistics()
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    nan, inf = float("nan"), float("inf")
    bad = [spec((0, 0, 0.0, 1.0)), spec((0, 1025, 0.0, 1.0)), spec((0, 16, 1.0, 1.0)), spec((0, 16, 2.0, 1.0)), spec((0, 16, nan, 1.0)),
           spec((0, 16, 0.0, nan)), spec((0, 16, 0.0, inf)), spec((7, 16, 0.0, 1.0)), spec((-1, 16, 0.0, 1.0)),
           spec((0, 16, -3.0e38, 3.0e38)), spec((0, 16, 0.0, 1.0), (0, 0, 0.0, 1.0))]
    for s in bad:
        assert L.sph_statistics(f._h, C.byref(out), s, len(s), hp) == -1, [(x.field, x.bins, x.lo, x.hi) for x in s]
        assert L.sph_last_error()
    five = spec(*[(0, 16, 0.0, 1.0)] * 5)
    assert L.sph_statistics(f._h, C.byref(out), five, 5, hp) == -1
    assert L.sph_statistics(f._h, C.byref(out), ok, -1, hp) == -1
    assert L.sph_statistics(f._h, None, None, 0, None) == -1                # null output
    assert L.sph_statistics(f._h, C.byref(out), None, 1, hp) == -1
    assert L.sph_statistics(f._h, C.byref(out), ok, 1, None) == -1
    assert L.sph_statistics_device(f._h, None, None, 0, None) == -1
    assert L.sph_statistics(None, C.byref(out), None, 0, None) == -1
    slab.close()
    _assert_equal_bits(pkg, f, "after the refusals")                        # the engine is still usable
    f.DispatchN(2)
    _assert_equal_bits(pkg, f, "after the refusals + 2")
    f.close()


# ---- 8. device variant ------------------------------------------------------------------------------------------------------------------
def test_device_variant_equals_the_host_variant(pkg):
    import torch
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.DispatchN(5)
    want = f.statistics(SPECS).tobytes()
    words = sum(b + 2 for _, b, _, _ in SPECS)
    dev = torch.full((C.sizeof(pkg.SphStatistics) // 8,), -1, dtype=torch.int64, device="cuda")
    dh = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    f.statistics_device(dev.data_ptr(), SPECS, dh.data_ptr())
    f.sync()
    assert dev.cpu().numpy().tobytes() + dh.cpu().numpy().tobytes() == want
    dev.fill_(-1)
    f.statistics_device(dev.data_ptr())                                     # no histograms
    f.sync()
    assert dev.cpu().numpy().tobytes() == want[:C.sizeof(pkg.SphStatistics)]
    f.close()


# ---- 9. the C++ example -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_run_monitor_example(pkg, tmp_path):
    exe = build_example(pkg, "run_monitor", tmp_path)
    res = run_example(exe, ["20", "50000"], timeout=300)
    assert res.returncode == 0 and "run_monitor OK" in res.stdout
    frames = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(frames) == 20
    for ln in frames:
        vals = dict(tok.split("=") for tok in ln.split()[2:])
        assert int(vals["counted"]) == 50000 and all(np.isfinite(float(v)) for v in vals.values()), ln
    res = run_example(exe, ["20", "50000", "1234"], timeout=300)          # poisons id 1234 after frame 3
    assert res.returncode != 0 and "id 1234" in res.stdout and "run_monitor OK" not in res.stdout
