"""The counting sort on the device (k_bin, k_scan_reduce / k_scan_blocksums / k_scan_apply, k_scatter, k_rank of csrc/sph_kernels.h)
on the scenes of grid_scenes.py, observed through the public surface only:

  * download_grid(): the histogram and every particle's cell, against oracle.build_grid;
  * the order inside the cells: neighbors(2 h, self_=True) equals neighbors_host, and the cell-mates in every particle's row stand in
    the oracle's `order` (a cell's diagonal, sqrt(3) h, is below 2 h, so every row holds the particle's whole cell);
  * DispatchN(2) byte-equal to oracle.substep.

Every assertion is on integers or bytes.  tests/test_grid_logic_cpu.py asserts that the scenes reach the alignments they claim."""
import numpy as np
import pytest

from conftest import assert_records_equal, to_oracle_params
import grid_scenes as GS
import rays_scenes as RS
import scalar_ref as SR
import tracer_ref as T
from support import engine, same_bits
from test_gpu_diffuse import _cfg, _host_step, _pair, _same_pool, _totals
from test_gpu_tracers import _same as same_tracers
import diffuse_ref as D

pytestmark = pytest.mark.gpu
F = np.float32

SEQUENCES = GS.sequences()
LAYOUTS = GS.layouts()


def _grid_equal(f, b, what):
    cnt, pcell = f.download_grid()
    assert np.array_equal(pcell, b["particle_cell"]), f"{what}: particle cells"
    assert np.array_equal(cnt, np.diff(b["cell_start"])), f"{what}: counts"


def _order_in_cells(pkg, f, rec, sp, b, what):
    """The neighbour rows at 2 h are the host's, and inside every row the members of the particle's own cell are the oracle's order."""
    R = float(F(2.0) * F(sp.param_h))
    off, idx = f.neighbors(R, self_=True)
    want_off, want_idx = pkg.neighbors_host(rec, sp, R, self_=True)
    assert np.array_equal(off, want_off), f"{what}: offsets differ from neighbors_host"
    assert np.array_equal(idx, want_idx), f"{what}: indices differ from neighbors_host"
    pcell, start, order = b["particle_cell"].astype(np.int64), b["cell_start"].astype(np.int64), b["order"].astype(np.int64)
    rows = np.repeat(np.arange(len(rec)), np.diff(off))
    mates = idx[pcell[idx] == pcell[rows]]
    length = (start[pcell + 1] - start[pcell])
    first = np.cumsum(length) - length
    want = order[np.repeat(start[pcell], length) + np.arange(length.sum()) - np.repeat(first, length)]
    assert np.array_equal(mates, want), f"{what}: the cell-mates of a row do not stand in (cell, id) order"


def _check_scene(pkg, oracle, rec, sp, passes, what, steps=2, order=True):
    op = to_oracle_params(oracle, sp)
    b = oracle.build_grid(rec, op)
    want = oracle.substep(rec, op, steps=steps)
    for kern in passes:
        f = engine(pkg, rec, sp, kern)
        _grid_equal(f, b, f"{what}, first build")                        # before any dispatch
        if order and kern == passes[0]:
            _order_in_cells(pkg, f, rec, sp, b, what)
        f.DispatchN(steps)
        assert_records_equal(f.download(), want, f"{what}, pass {kern}, {steps} substeps")
        _grid_equal(f, oracle.build_grid(want, op), f"{what}, pass {kern}, build after {steps} substeps")
        f.close()


# ---- A: run shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_run_shapes(pkg, oracle, name):
    """k_bin's runs at the first build: every run length at every start lane, every lane a head, a cell met again by the same wave
    and by later blocks, falling cell order."""
    rec, sp = GS.from_cells(pkg, GS.RUN_DIMS, SEQUENCES[name], 3)
    _check_scene(pkg, oracle, rec, sp, (3,), name)


# ---- B: rank alignments --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_rank_alignments(pkg, oracle, name):
    """k_rank: cells of 1 .. 300 members beginning at slot offsets 0, 1, 31, 62, 63 mod 64 in a shuffled upload order."""
    rec, sp = GS.from_cells(pkg, GS.RUN_DIMS, LAYOUTS[name][2], 3)
    _check_scene(pkg, oracle, rec, sp, (3, 2, 1), name)


# ---- C: scan seams -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GS.SMALL_GRIDS + GS.LARGE_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_scan_seams(pkg, oracle, dims):
    """The residues of scan_load16's tail, one and two tiles, 1024 tiles (the last fused scan) and 1025 (k_scan_blocksums), with
    members on both sides of the seams."""
    rec, sp = GS.from_cells(pkg, dims, GS.seam_scene_cells(dims, 7), 7)
    _check_scene(pkg, oracle, rec, sp, (3,), f"grid {dims}", order=int(np.prod(dims)) <= 2 * GS.SCAN_TILE)


TWIN_GRIDS = ((3, 11, 62), (3, 5, 137), (160, 160, 82))


@pytest.mark.parametrize("dims", TWIN_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_scan_seams_tracer_sort(pkg, oracle, dims):
    """The tracers' cell sort scans the same number of cells: one set_tracers and one dispatch against tracer_ref."""
    rec, sp = GS.from_cells(pkg, dims, GS.seam_scene_cells(dims, 7), 7)
    C = int(np.prod(dims))
    rng = np.random.default_rng(8)
    rec["vel"][:, :3] = rng.normal(0.0, 1.0, (len(rec), 3)).astype(F)    # a field that moves the tracers
    cells = np.concatenate([rng.integers(0, C, 400), GS.seam_cells(C)[:200], GS.seam_cells(C)[-200:]])
    p4 = np.concatenate([GS.cell_points(pkg, sp, cells, 9), rng.random((len(cells), 1)).astype(F)], axis=1)
    op = to_oracle_params(oracle, sp)
    want, want_rec = T.run(oracle, rec, op, p4, 1, T.MIDPOINT)
    assert (want["pos"] != p4[:, :3]).any(axis=1).sum() > 100
    f = engine(pkg, rec, sp)
    f.set_tracers(p4, T.MIDPOINT)
    f.DispatchCompute()
    same_tracers(f.tracers(), want, f"grid {dims}")
    assert_records_equal(f.download(), want_rec, f"grid {dims}: records beside tracers")
    f.close()


@pytest.mark.parametrize("dims", TWIN_GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_scan_seams_ray_sort(pkg, dims):
    """The cell-ordered cast (SPH_OPT_RAYS_VARIANT 1) scans numCells + 1 counts: against rays_host, the definition."""
    rec, sp = GS.from_cells(pkg, dims, GS.seam_scene_cells(dims, 7), 7)
    g = pkg.compute_grid_extents(sp)
    rng = np.random.default_rng(10)
    lo = np.array(list(g.gridMin), F)
    ext = F(g.cellSize) * np.array(list(g.dims), F)
    o = lo + rng.random((600, 3)).astype(F) * ext                        # origins in every part of the grid, some rays leave it
    o[:100] -= F(0.75)
    r = RS.rays(o, (rng.random((600, 3)).astype(F) - F(0.5)), 0.0, 40.0)
    radius = 0.5 * sp.param_h
    want = pkg.rays_host(rec, sp, r, radius, with_info=True)
    assert 50 < want[4].hits < 600
    f = engine(pkg, rec, sp)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 1)
    RS.same_hits(f.raycast(r, radius), want, f"grid {dims}")
    assert f.rays_info().hits == want[4].hits
    f.close()


@pytest.mark.parametrize("capacity", [2047, 2048, 2049])
def test_scan_seams_diffuse_pool(pkg, oracle, capacity):
    """The diffuse pool's scan runs over the pool capacity: one tile less one, one tile, one tile and one."""
    rec, sp, _, pool = D.scene(pkg, oracle)
    cfg = _cfg(pkg, capacity=capacity)
    f, h = _pair(pkg, rec, sp, cfg, pool[:capacity])
    pool = pool[:capacity]
    totals = _totals(pool)
    for i in range(10):                                                  # (the pool is full after nine substeps)
        f.DispatchCompute()
        pool, totals = _host_step(pkg, h, cfg, pool, totals)
        _same_pool(f, pool, totals, f"C = {capacity}, substep {i}")
    assert totals["alive"] == capacity and totals["dropped"] > 0
    f.close()
    h.close()


# ---- D: axis limits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_of_1024_cells(pkg, oracle, axis):
    """Cell coordinates up to 1023 in the 10-bit fields k_rank packs and the passes decode: three lattice patches at both ends and in
    the middle of the long axis, three substeps with every pass."""
    rec, sp, patches = GS.axis_patches(pkg, axis)
    op = to_oracle_params(oracle, sp)
    b = oracle.build_grid(rec, op)
    coord = (b["particle_cell"] // int(np.prod(b["grid"].dims[:axis]))) % 1024
    assert [sorted(set(coord[p].tolist())) for p in patches] == [[0, 1, 2], [510, 511, 512, 513], [1021, 1022, 1023]]
    want = oracle.substep(rec, op, steps=3)
    for p in patches:
        assert (want["pressure"][p] > 0).any(), "the patch's particles did not interact"
    for kern in (3, 2, 1):
        f = engine(pkg, rec, sp, kern)
        _grid_equal(f, b, f"axis {axis}")
        f.DispatchN(3)
        assert_records_equal(f.download(), want, f"axis {axis} pass {kern}")
        f.close()


def test_axis_of_1024_cells_scalars(pkg, oracle):
    """sph_scalar.h decodes the same cell bits: two substeps of diffusion against scalar_ref.step32, bit for bit."""
    rec, sp, patches = GS.axis_patches(pkg, 0)
    op = to_oracle_params(oracle, sp)
    c = np.random.default_rng(5).uniform(-1.0, 2.0, (len(rec), 2)).astype(F)
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0)
    Dk, lam = np.array([1.0, 0.4], F) * F(0.4 / float(s1)), np.array([0.0, 2.0], F)
    cur, state = c, rec
    for _ in range(2):
        b = oracle.build_grid(state, op)
        cur, _ = SR.step32(state, cur, sp.param_h, sp.param_mass, Dk, lam, sp.param_timeStep, b["grid"], b["cell_start"], b["order"])
        state = oracle.substep(state, op)
    for p in patches:
        assert (cur[p] != c[p]).any()
    f = engine(pkg, rec, sp)
    f.set_scalars(c, diffusivity=Dk, decay=lam)
    f.DispatchN(2)
    same_bits(f.scalars(), cur, "scalars on a grid of 1024 x 3 x 3")
    assert_records_equal(f.download(), state, "records beside scalars")
    f.close()


def test_axis_of_1025_cells_is_refused(pkg, oracle):
    """One cell more than the 10 bits hold: an error at dispatch, before any launch; the engine works on once the member is back."""
    rec, sp, _ = GS.axis_patches(pkg, 0)
    op = to_oracle_params(oracle, sp)
    f = engine(pkg, rec, sp)
    f.DispatchCompute()
    good = list(sp.param_boxHalf)
    f.grid_cap = 1025
    f.param_boxHalf = (GS.H * ((1025 - 2) / 2.0 - 0.25), good[1], good[2])
    assert pkg.compute_grid_extents(f.params).dims[0] == 1025
    with pytest.raises(pkg.SphError, match="10 bits"):
        f.DispatchCompute()
    f.param_boxHalf = tuple(good)
    f.grid_cap = 1024
    f.DispatchCompute()
    assert_records_equal(f.download(), oracle.substep(rec, op, steps=2), "after the refusal")
    f.close()


# ---- E: one engine, changing grids ---------------------------------------------------------------------
def test_one_engine_changing_grids(pkg, oracle):
    """param_boxHalf edited between calls: two million cells, 27, then 4096 cells as (4, 8, 128) and as (8, 16, 32) (the same
    buffers, other dims: the histogram must already be clean), and two million again.  After every edit the grid and one substep."""
    chain = ((160, 160, 82), (3, 3, 3), (4, 8, 128), (8, 16, 32), (160, 160, 82))
    rec, sp = GS.from_cells(pkg, chain[0], GS.seam_scene_cells(chain[0], 11)[:3000], 11)
    f = engine(pkg, rec, sp)
    want = rec
    for i, dims in enumerate(chain):
        f.param_boxHalf = tuple(GS.params(pkg, dims).param_boxHalf)
        assert tuple(pkg.compute_grid_extents(f.params).dims) == dims
        op = to_oracle_params(oracle, f.params)
        _grid_equal(f, oracle.build_grid(want, op), f"edit {i}: grid {dims}")
        f.DispatchCompute()
        want = oracle.substep(want, op)
        assert_records_equal(f.download(), want, f"edit {i}: grid {dims}, one substep")
    f.close()
