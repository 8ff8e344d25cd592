"""The numpy restatement of the state statistics (tests/stats_ref.py) against exact arithmetic and plain numpy,
the histogram's edge cases, and the layout of the ctypes mirror against include/sph_abi.h.  No GPU.

Bound for an fp64 sum against math.fsum of the same terms: gamma_d * fsum(|terms|), gamma_d = d u / (1 - d u), u = 2^-53,
d = depth of the tree (11 levels inside a tile of 2048 + log2 of the padded tile count: every term passes through at most that many
additions, each with relative error <= u; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, pairwise summation)
plus the roundings inside one term: 2 for (vx*vx + vy*vy) + vz*vz (the products of two converted fp32 values are exact in fp64),
1 for 1 / rho, 0 for rho * rho (exact), 5 for a component of (x - c) x v (two differences, two products, one difference), 0 for a
converted fp32 value.  Derived, not measured."""
import ctypes as C
import math
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, small_scene
import stats_ref
from support import c_layout

G = os.path.join(ROOT, "tests", "golden")
F = np.float32
U = 2.0 ** -53


def _states(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    yield "settled_pool", fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    z = np.load(os.path.join(G, "scene4096.npz"))
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    yield "scene4096 after_100", z["after_100"], sp
    c = np.load(os.path.join(G, "cylinder2000.npz"))
    yield "cylinder2000", c["after"], pkg.default_params(param_shapeType=2, param_boxHalf=(2.2, 1.6, 0.9), param_boxEulerDeg=(10.0, -25.0, 40.0),
                                                         param_boxCenter=(0.2, -0.1, 0.3), param_mass=float(c["mass"]))


def _run(pkg, rec, sp, specs=()):
    g = pkg.compute_grid_extents(sp)
    return stats_ref.statistics(rec, sp, g, stats_ref.host_cells(rec, g), specs), g


def test_sums_against_exact_arithmetic(pkg):
    for name, rec, sp in _states(pkg):
        ref, _ = _run(pkg, rec, sp)
        _, _, _, _, _, counted = stats_ref.sets(rec)
        t = stats_ref.terms(rec, counted, sp.param_boxCenter)
        for k in stats_ref.SUM_NAMES:
            d = stats_ref.tree_depth(len(rec)) + stats_ref.TERM_ROUNDINGS[k]
            bound = d * U / (1 - d * U) * math.fsum(np.abs(t[k]))
            err = abs(float(ref["sums"][k]) - math.fsum(t[k]))
            assert err <= bound, (name, k, err, bound)
            if name == "settled_pool" and k == "speed2":
                assert 0 < bound < 1e-10 and err < 1e-11                       # the bound is not vacuous: about 5e-11 on a sum of 28860.8
                assert abs(float(ref["sums"][k]) - 28860.802002803) < 1e-8


def test_tree_is_the_written_halving_loop():
    rng = np.random.default_rng(1)
    for n in (0, 1, 5, 2047, 2048, 2049, 3 * 2048 + 17, 5 * 2048):
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        nt = -(-n // 2048)
        tiles = []
        for t in range(nt):
            y = np.zeros(2048)
            seg = x[2048 * t:2048 * (t + 1)]
            y[:len(seg)] = seg
            s = 1024
            while s >= 1:
                for i in range(s):
                    y[i] += y[i + s]
                s //= 2
            tiles.append(y[0])
        t2 = 1
        while t2 < nt:
            t2 *= 2
        y = np.zeros(t2)
        y[:nt] = tiles
        s = t2 // 2
        while s >= 1:
            for i in range(s):
                y[i] += y[i + s]
            s //= 2
        want = y[0] if nt else 0.0
        assert np.float64(stats_ref.tree_sum(x)).tobytes() == np.float64(want).tobytes(), n
    assert stats_ref.tree_depth(50000) == 11 + 5 and stats_ref.tree_depth(4194304) == 22 and stats_ref.tree_depth(100) == 11


def test_order_matters_and_the_canonical_order_is_cell_then_id(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    rec, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    ref, g = _run(pkg, rec, sp)
    perm = np.random.default_rng(5).permutation(len(rec))
    shuffled = rec[perm]                                                        # other ids: other order inside the cells, other sums' bits
    cells = stats_ref.host_cells(rec, g)
    order = np.lexsort((np.arange(len(rec)), cells))
    assert np.all(np.diff(cells[order]) >= 0)
    same = cells[order][1:] == cells[order][:-1]
    assert np.all(np.diff(order)[same] > 0)
    _, _, _, _, _, counted = stats_ref.sets(rec)
    t = stats_ref.terms(rec, counted, sp.param_boxCenter)["speed2"]
    assert float(ref["sums"]["speed2"]) == float(stats_ref.tree_sum(t[order]))
    ref2, _ = _run(pkg, shuffled, sp)
    assert ref2["numCounted"] == ref["numCounted"] and ref2["maxDensity"][0] == ref["maxDensity"][0]
    assert np.array_equal(ref2["occupancy"], ref["occupancy"])


def test_extrema_counts_and_occupancy_against_plain_numpy(pkg):
    for name, rec, sp in _states(pkg):
        ref, g = _run(pkg, rec, sp)
        assert ref["numRecords"] == ref["numFluid"] == ref["numCounted"] == len(rec) and ref["numNonFinite"] == 0, name
        for a in range(3):
            assert ref[f"minPos{a}"] == (rec["pos"][:, a].min(), int(np.argmin(rec["pos"][:, a]))), name
            assert ref[f"maxPos{a}"] == (rec["pos"][:, a].max(), int(np.argmax(rec["pos"][:, a]))), name
        assert ref["minDensity"] == (rec["density"].min(), int(np.argmin(rec["density"]))), name
        assert ref["maxPressure"] == (rec["pressure"].max(), int(np.argmax(rec["pressure"]))), name
        v = rec["vel"]
        s2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        assert ref["maxSpeed2"] == (s2.max(), int(np.argmax(s2))) and ref["maxSpeed"] == np.sqrt(s2.max()), name
        occ = np.bincount(stats_ref.host_cells(rec, g), minlength=g.numCells)
        assert ref["occupiedCells"] == np.count_nonzero(occ) and ref["maxCellCount"] == occ.max() and ref["maxCellIndex"] == np.argmax(occ), name
        assert int(ref["occupancy"].sum()) == g.numCells and int((ref["occupancy"] * np.arange(65)).sum()) <= len(rec), name
        for m in range(64):
            assert ref["occupancy"][m] == np.count_nonzero(occ == m), (name, m)
        assert ref["occupancy"][64] == np.count_nonzero(occ >= 64), name
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    assert set(fx["settled"]["isActive"]) == {0}                                # so isActive must not enter the definition of fluid


def test_tie_rule_lowest_id_and_stored_bits(pkg):
    rec, sp = small_scene(pkg, n=300, grid=8, seed=3)
    P = rec.copy()
    P["density"][:] = F(1000.0)
    P["density"][[40, 7, 299]] = F(2500.0)                                      # the maximum, three times
    P["pressure"][:] = F(5.0)
    P["pressure"][[100, 20]] = [F(0.0), F(-0.0)]                                # compare equal: id 20 wins, and its bits (-0.0) are reported
    ref, _ = _run(pkg, P, sp)
    assert ref["maxDensity"] == (F(2500.0), 7)
    assert ref["minDensity"] == (F(1000.0), 0)
    assert ref["minPressure"][1] == 20 and np.signbit(ref["minPressure"][0])
    s = stats_ref.pack(ref, pkg.SphStatistics)
    assert np.signbit(F(s.minPressure.value)) and s.minPressure.id == 20 and s.maxDensity.id == 7
    P["pressure"][[100, 20]] = [F(-0.0), F(0.0)]
    ref, _ = _run(pkg, P, sp)
    assert ref["minPressure"][1] == 20 and not np.signbit(ref["minPressure"][0])


def test_empty_counted_set_and_no_particles(pkg):
    rec, sp = small_scene(pkg, n=300, grid=8, seed=3)
    P = rec.copy()
    P["isGhost"] = 1
    P["isActive"][:100] = 1
    n_all = len(P)
    ref, g = _run(pkg, P, sp, [(stats_ref.DENSITY, 4, 0.0, 1.0)])
    assert (ref["numFluid"], ref["numActiveGhosts"], ref["numInactiveGhosts"], ref["numOther"], ref["numCounted"]) == (0, 100, n_all - 100, 0, 0)
    assert ref["minDensity"] == (np.inf, 0xFFFFFFFF) and ref["maxDensity"] == (-np.inf, 0xFFFFFFFF) and ref["maxSpeed"] == 0
    assert all(float(v) == 0.0 and not np.signbit(v) for v in ref["sums"].values())
    assert ref["firstNonFiniteId"] == ref["firstEscapedId"] == 0xFFFFFFFF and ref["histograms"][0].sum() == 0
    assert ref["occupiedCells"] > 0                                             # the grid holds every record, ghosts included
    ref, _ = _run(pkg, P[:0], sp)
    assert ref["numRecords"] == 0 and ref["occupiedCells"] == 0 and ref["maxCellCount"] == 0 and ref["maxCellIndex"] == 0
    assert ref["occupancy"][0] == g.numCells and float(ref["sums"]["density"]) == 0.0
    assert len(bytes(stats_ref.pack(ref, pkg.SphStatistics))) == 832


def test_injected_nan_inf_and_escaped_records(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    g = pkg.compute_grid_extents(sp)
    cells = stats_ref.host_cells(rec, g)
    P = rec.copy()
    a, b, c = 700, 1900, 3000
    P["vel"][a, 1] = np.nan
    P["density"][b] = np.inf
    P["pos"][c, :3] = (50.0, 60.0, -70.0)
    P["padA"][3500] = -np.inf
    P["isGhost"][3600] = 1
    P["pos"][3600, 0] = np.nan                                                  # a ghost is not a non-finite FLUID record
    cells[c] = stats_ref.host_cells(P[c:c + 1], g)[0]
    ref = stats_ref.statistics(P, sp, g, cells, [(stats_ref.POS_X, 8, -3.0, 3.0)])
    assert ref["numNonFinite"] == 3 and ref["firstNonFiniteId"] == a and ref["numCounted"] == len(P) - 4
    assert ref["numEscaped"] == 1 and ref["firstEscapedId"] == c
    assert ref["maxPos1"] == (F(60.0), c) and ref["minPos2"] == (F(-70.0), c)
    assert all(np.isfinite(float(v)) for v in ref["sums"].values())
    keep = np.ones(len(P), bool)
    keep[[a, b, 3500, 3600]] = False
    assert abs(float(ref["sums"]["density"]) - math.fsum(P["density"][keep].astype(np.float64))) <= 20 * U * math.fsum(P["density"][keep].astype(np.float64))
    assert ref["histograms"][0].sum() == ref["numCounted"] and ref["histograms"][0][9] >= 1          # x = 50 lies at or above hi


def test_histogram_edge_cases():
    h = stats_ref.histogram
    lo, hi = F(0.0), F(1.0)
    assert list(h([lo], 4, lo, hi)) == [0, 1, 0, 0, 0, 0]                       # v == lo: the first bin
    assert list(h([hi], 4, lo, hi)) == [0, 0, 0, 0, 0, 1]                       # v == hi: the slot above
    assert list(h([np.nextafter(lo, F(-1))], 4, lo, hi)) == [1, 0, 0, 0, 0, 0]
    # the value just below hi whose scaled index rounds up to `bins`: (v - lo) * scale == bins in fp32, clamped into the last bin
    found = [(l, hh, n) for l, hh, n in ((F(-1.9338895082473755), F(0.5077885389328003), 42), (F(-1.8656576871871948), F(0.3260120153427124), 878), (F(0.0), F(3.0), 3))
             if np.floor((np.nextafter(hh, F(-9)) - l) * (F(n) / (hh - l))) >= n]
    assert len(found) >= 2, "no case where the scaled index rounds up to bins"  # (found by a random search; exact in fp32, so they stay cases)
    for l, hh, n in found:
        out = h([np.nextafter(hh, F(-9))], n, l, hh)
        assert out[n] == 1 and out.sum() == 1
    assert list(h([-5.0, 0.0, 0.5, 0.999, 1.0, 7.0], 1, lo, hi)) == [1, 3, 2]   # bins == 1
    rng = np.random.default_rng(2)
    v = rng.normal(0.5, 0.4, 20000).astype(F)
    got = h(v, 37, F(-0.25), F(1.5))
    idx = np.floor((v.astype(F) - F(-0.25)) * (F(37) / (F(1.5) - F(-0.25)))).astype(np.int64)
    want = np.bincount(np.where(v < F(-0.25), 0, np.where(v >= F(1.5), 38, 1 + np.minimum(idx, 36))), minlength=39)
    assert np.array_equal(got, want) and got.sum() == len(v)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_ctypes_mirror_matches_the_header(pkg, tmp_path):
    """sizeof and every offsetof of SphStatistics / SphStatExtremum / SphHistogramSpec, printed by C99 compiled against the header."""
    structs = {"SphStatistics": pkg.SphStatistics, "SphStatExtremum": pkg.SphStatExtremum, "SphHistogramSpec": pkg.SphHistogramSpec}
    enum = ('printf("enum %d %d %d %d %d %d %d %d %d\\n", SPH_STAT_DENSITY, SPH_STAT_PRESSURE, SPH_STAT_SPEED, SPH_STAT_POS_X, SPH_STAT_POS_Y,'
            ' SPH_STAT_POS_Z, SPH_STAT_FOAM, SPH_STAT_MAX_SPECS, SPH_STAT_MAX_BINS);')
    seen = 0
    for sname, st in structs.items():
        size, offsets, extra = c_layout(sname, st, [enum], tmp_path)
        assert size == C.sizeof(st), sname
        assert [f for f, _ in offsets] == [f for f, _ in st._fields_], sname
        for fname, val in offsets:
            assert val == getattr(st, fname).offset, (sname, fname, val)
        seen += 1 + len(offsets)
        assert len(extra) == 1
    assert seen == sum(len(st._fields_) + 1 for st in structs.values())
    assert C.sizeof(pkg.SphStatistics) == 832 and C.sizeof(pkg.SphStatistics) % 8 == 0 and C.alignment(pkg.SphStatistics) == 8
    assert C.sizeof(pkg.SphHistogramSpec) == 16
    assert extra[0].split()[1:] == [str(v) for v in (pkg.SPH_STAT_DENSITY, pkg.SPH_STAT_PRESSURE, pkg.SPH_STAT_SPEED, pkg.SPH_STAT_POS_X, pkg.SPH_STAT_POS_Y,
                                                     pkg.SPH_STAT_POS_Z, pkg.SPH_STAT_FOAM, pkg.SPH_STAT_MAX_SPECS, pkg.SPH_STAT_MAX_BINS)]
    assert (stats_ref.DENSITY, stats_ref.PRESSURE, stats_ref.SPEED, stats_ref.POS_X, stats_ref.POS_Y, stats_ref.POS_Z, stats_ref.FOAM) == tuple(range(7))
    # the header names every member the mirror has, in the same order
    hdr = open(os.path.join(ROOT, "include", "sph_abi.h")).read()
    body = re.search(r"typedef struct SphStatistics \{(.*?)\} SphStatistics;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*[,;]", body)
    assert names == [f for f, _ in pkg.SphStatistics._fields_]


def test_the_two_entry_points_are_in_the_symbol_list(pkg):
    assert "sph_statistics" in pkg.ABI_SYMBOLS and "sph_statistics_device" in pkg.ABI_SYMBOLS
    L = pkg.load_library()
    assert hasattr(L, "sph_statistics") and hasattr(L, "sph_statistics_device")
    assert hasattr(pkg.SPHFluidGPU, "statistics") and hasattr(pkg.SPHFluidGPU, "statistics_device")


def test_derived_numbers_of_the_python_mirror(pkg):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    rec, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    ref, _ = _run(pkg, rec, sp)
    st = pkg.Statistics(stats_ref.pack(ref, pkg.SphStatistics), [], sp)
    m = float(sp.param_mass)
    v = rec["vel"][:, :3].astype(np.float64)
    assert st.kinetic_energy == pytest.approx(0.5 * m * (v * v).sum(), rel=1e-12)
    assert st.center_of_mass == pytest.approx(rec["pos"][:, :3].astype(np.float64).mean(axis=0), abs=1e-9)
    assert st.mean_density == pytest.approx(rec["density"].astype(np.float64).mean(), rel=1e-12)
    assert st.std_density == pytest.approx(rec["density"].astype(np.float64).std(), rel=1e-9)
    assert st.cfl == pytest.approx(float(ref["maxSpeed"]) * float(sp.param_timeStep) / float(sp.param_h))
    assert st.volume == pytest.approx(m * (1.0 / rec["density"].astype(np.float64)).sum(), rel=1e-12)
    assert st.potential_energy == pytest.approx(-m * float(sp.param_gravityY) * rec["pos"][:, 1].astype(np.float64).sum(), rel=1e-12)
    assert st.ok and st.numCounted == len(rec) and st.bounding_box[0][1] == rec["pos"][:, 1].min()
    assert st.mean_density / float(sp.param_restDensity) > 4                    # the compressed pool of DESIGN.md section 11
