"""k_sph_walk's memory access classes (window staging loads through the bounded buffer resource, the target's own loads, the
cellStart run bounds, the walks' gathers, the output stores) on the shapes at which each of them takes another path.

A cache policy moves the same bytes, so every case compares ALL record bytes of SPH_OPT_NEIGHBOR_KERNEL 3 (k_sph_walk) with
kernel 1 (k_sph_slow: plain loads and stores) after 3 substeps, and reads the walk's debug counters (SPH_OPT_DEBUG 8) to make
sure that the path the case is about did run."""
import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
from support import records

pytestmark = pytest.mark.gpu

F = np.float32
H = 0.28
STEPS = 3


def _params(pkg, grid):
    syn = pkg.synthetic
    return pkg.default_params(**syn.params_fields(syn.BenchConfig(99, "walk policy", 0, tuple(grid), 0.85, 1)))


def _in_cells(pkg, sp, cells, per_cell, seed, spread=0.3):
    """per_cell particles in each of the given (cx, cy, cz) cells, within +-spread * h of the cell's centre."""
    g = pkg.compute_grid_extents(sp)
    rng = np.random.default_rng(seed)
    lo = np.array([g.gridMin[0], g.gridMin[1], g.gridMin[2]], np.float64)
    cells = np.repeat(np.asarray(cells, np.float64), per_cell, axis=0)
    pos = lo + (cells + 0.5 + rng.uniform(-spread, spread, cells.shape)) * float(g.cellSize)
    rec = records(pkg, pos.astype(F), np.zeros_like(pos, dtype=F))
    got = np.floor((rec["pos"][:, :3].astype(np.float64) - lo) / float(g.cellSize))
    assert (got == cells).all()                           # every particle sits in the cell it was meant for
    return rec[rng.permutation(len(rec))]


def _walk_vs_slow(pkg, rec, sp, what):
    """3 substeps with k_sph_walk (debug counters on) and with k_sph_slow: all record bytes equal.  Returns the walk's counters."""
    outs, counters = [], None
    for kern in (3, 1):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        f.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, kern)
        if kern == 3:
            f.set_option(pkg.SPH_OPT_DEBUG, 8)
        f.DispatchN(STEPS)
        outs.append(f.download())
        if kern == 3:
            counters = f.debug_counters(reset=True)
        f.close()
    print(what, {k: counters[k] for k in ("rows", "rows_unstaged", "slow_targets", "overflow_targets", "far_targets", "lanes", "list_entries")})
    assert_records_equal(outs[0], outs[1], f"{what}: k_sph_walk vs k_sph_slow after {STEPS} substeps")
    assert counters["lanes"] >= STEPS * len(rec) and counters["rows"] > 0      # the walk kernel did run, over every slot
    return counters


def test_partly_live_last_wave(pkg):
    """4001 particles = 15 blocks of 256 + 161 = 62 waves + 33 lanes: the lanes past the end stay for the staging and own nothing."""
    rec, sp = small_scene(pkg, n=4001, grid=16, seed=11)
    assert len(rec) % 64 and len(rec) % 256
    c = _walk_vs_slow(pkg, rec, sp, "4001 particles")
    assert c["rows_unstaged"] < c["rows"]                 # windows were staged


@pytest.mark.parametrize("per_cell, staged", [(48, True), (49, False)])
def test_line_of_three_cells_fills_the_window(pkg, per_cell, staged):
    """Three neighbouring cells along x with 48 particles each: every wave's window of that row is exactly the 144 slots the LDS
    window holds (loads past its end return 0 through the bounded resource) and is staged.  With 49 per cell it is 147 slots and
    the row is walked from global memory."""
    sp = _params(pkg, (10, 8, 8))
    rec = _in_cells(pkg, sp, [(4, 4, 4), (5, 4, 4), (6, 4, 4)], per_cell, seed=per_cell)
    c = _walk_vs_slow(pkg, rec, sp, f"3 cells x {per_cell}")
    if staged:
        assert c["rows_unstaged"] == 0
    else:
        assert c["rows_unstaged"] > 0


def test_edge_and_corner_cells(pkg):
    """Particles only in corner and edge cells of the grid: most of their nine candidate rows fall outside it."""
    gx, gy, gz = 9, 7, 6
    sp = _params(pkg, (gx, gy, gz))
    cells = [(x, y, z) for x in (0, gx - 1) for y in (0, gy - 1) for z in (0, gz - 1)]                       # corners
    cells += [(4, 0, 0), (4, gy - 1, gz - 1), (0, 3, 0), (gx - 1, 3, gz - 1), (0, 0, 3), (gx - 1, gy - 1, 2), (1, 0, 0), (gx - 2, gy - 1, gz - 1)]
    rec = _in_cells(pkg, sp, cells, 7, seed=5)
    assert len(rec) % 64
    c = _walk_vs_slow(pkg, rec, sp, "edge and corner cells")
    assert c["rows"] < 9 * c["lanes"] // 64               # some waves met rows without candidates (outside the grid or empty)


def test_single_particle(pkg):
    sp = _params(pkg, (8, 8, 8))
    rec = _in_cells(pkg, sp, [(3, 4, 2)], 1, seed=1)
    c = _walk_vs_slow(pkg, rec, sp, "n = 1")
    assert c["list_entries"] == 0 and c["slow_targets"] == 0


def test_all_in_one_cell(pkg):
    """300 particles in one cell: window offsets exceed the 8 bits of a list entry, the exact sweeps take over."""
    sp = _params(pkg, (8, 8, 8))
    rec = _in_cells(pkg, sp, [(4, 3, 4)], 300, seed=2, spread=0.45)
    c = _walk_vs_slow(pkg, rec, sp, "300 in one cell")
    assert c["rows_unstaged"] > 0 and c["slow_targets"] >= len(rec)           # at least the whole first substep fell back


# What the parent commit of the cache-policy change reports for this input (3 substeps, SPH_OPT_DEBUG 8): slow_targets = 0.
LATTICE_FALLBACK_TARGETS_BEFORE = 0


def test_config1_lattice(pkg):
    """BASELINE.json configs[0]: the jittered lattice of 32 768 particles in 32^3 cells, the regime the benchmark times: every
    window staged, every target on its list."""
    syn = pkg.synthetic
    cfg = syn.CONFIGS[1]
    rec, _ = syn.make_particles(cfg)
    assert len(rec) == 32768
    sp = pkg.default_params(**syn.params_fields(cfg))
    c = _walk_vs_slow(pkg, rec, sp, "config 1")
    assert c["slow_targets"] <= LATTICE_FALLBACK_TARGETS_BEFORE
    assert c["rows_unstaged"] == 0 and c["list_entries"] > 0
