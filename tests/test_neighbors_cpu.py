"""Neighbour lists on the CPU (sph_neighbors_host: the kernels' accept function over a counting sort of its own) against the float64
brute force of neighbors_ref.py, the flags, query rows, argument errors and the layout of SphNeighborInfo.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import neighbors_ref as NR
import support

F = np.float32
# random_scene seeds with every particle strictly inside the grid box and, at all five radii, no pair within 1e-6 R^2 of the sphere
# (both asserted below)
SEEDS = (1, 3, 6, 15)
FACTORS = (0.5, 1.0, 1.5, 2.5, 3.0)


def _scene(pkg, seed):
    rec, sp, _, what = support.random_scene(pkg, seed)
    return rec, sp, what


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("seed", SEEDS)
def test_host_lists_equal_brute_force(pkg, seed, factor):
    rec, sp, what = _scene(pkg, seed)
    assert NR.inside_grid(pkg, rec["pos"], sp), what
    R = float(F(factor * sp.param_h))
    off, idx, margin = NR.brute_force(pkg, rec["pos"], sp, R)
    print(what, "R", R, "pairs", off[-1], "margin", margin)
    assert margin > 1e-6, "fixture condition: a pair sits on the sphere within rounding"
    got_off, got_idx = pkg.neighbors_host(rec, sp, R)
    assert got_off.dtype == np.int64 and got_idx.dtype == np.int32
    assert np.array_equal(got_off, off) and np.array_equal(got_idx, idx)
    assert off[-1] > 0


@pytest.mark.parametrize("seed", SEEDS[:2])
def test_flags(pkg, seed):
    rec, sp, what = _scene(pkg, seed)
    R = float(F(1.5 * sp.param_h))
    n = len(rec)
    off, idx = pkg.neighbors_host(rec, sp, R)
    # SELF: the default rows with the particle itself, by identity
    soff, sidx, m = NR.brute_force(pkg, rec["pos"], sp, R, self_=True)
    assert m > 1e-6
    g_off, g_idx = pkg.neighbors_host(rec, sp, R, self_=True)
    assert np.array_equal(g_off, soff) and np.array_equal(g_idx, sidx)
    assert np.array_equal(np.diff(g_off), np.diff(off) + 1)
    for i, (a, b) in enumerate(zip(NR.rows_of(g_off, g_idx), NR.rows_of(off, idx))):
        assert np.array_equal(a[a != i], b) and (a == i).sum() == 1
    # HALF: id_j > id_i only; with the transposes, the default lists
    h_off, h_idx = pkg.neighbors_host(rec, sp, R, half=True)
    boff, bidx, _ = NR.brute_force(pkg, rec["pos"], sp, R, half=True)
    assert np.array_equal(h_off, boff) and np.array_equal(h_idx, bidx)
    assert h_off[-1] * 2 == off[-1]
    rows = np.repeat(np.arange(n), np.diff(h_off))
    assert (h_idx > rows).all()
    fwd, back = NR.transpose_pairs(h_off, h_idx)
    assert np.array_equal(np.sort(np.concatenate([fwd, back])), NR.transpose_pairs(off, idx)[0])
    # COUNT_ONLY: the same offsets, no indices
    c_off, c_idx = pkg.neighbors_host(rec, sp, R, count_only=True)
    assert c_idx is None and np.array_equal(c_off, off)
    # symmetry, bit for bit
    fwd, back = NR.transpose_pairs(off, idx)
    assert np.array_equal(fwd, back)


def test_symmetry_with_clamped_cells_ghosts_and_nan(pkg):
    """Particles outside the grid box land in clamped cells, ghosts and inactive records are binned like any other record, a NaN
    position is accepted by nobody: the relation stays symmetric at every stencil width."""
    rng = np.random.default_rng(5)
    sp = pkg.default_params(param_h=0.5, param_boxHalf=(1.5, 1.0, 1.25), grid_cap=160)
    g = pkg.compute_grid_extents(sp)
    lo = np.array(list(g.gridMin), F)
    ext = np.array(list(g.dims), F) * F(g.cellSize)
    n = 900
    pos = lo + (rng.random((n, 3)).astype(F) * F(1.6) - F(0.3)) * ext       # 30 % of the box beyond every face
    rec = support.records(pkg, pos, np.zeros((n, 3), F), ghost=(np.arange(n) % 7 == 0).astype(np.int32))
    rec["isActive"] = (np.arange(n) % 5 != 0)
    rec["pos"][17, 1] = np.nan
    rec["pos"][400, 0] = np.inf
    for fac in (1.0, 2.0, 3.0):
        off, idx = pkg.neighbors_host(rec, sp, fac * sp.param_h)
        fwd, back = NR.transpose_pairs(off, idx)
        assert np.array_equal(fwd, back) and len(idx)
        assert off[18] == off[17] and off[401] == off[400] and not np.isin(idx, (17, 400)).any()
        s_off, s_idx = pkg.neighbors_host(rec, sp, fac * sp.param_h, self_=True)
        assert s_off[18] - s_off[17] == 1 and s_idx[s_off[17]] == 17            # SELF is by slot identity, not by distance


def test_query_rows(pkg):
    rec, sp, what = _scene(pkg, SEEDS[2])
    R = float(F(sp.param_h))
    s_off, s_idx = pkg.neighbors_host(rec, sp, R, self_=True)
    pts = rec["pos"].copy()
    q_off, q_idx = pkg.neighbors_host(rec, sp, R, points=pts)
    assert np.array_equal(q_off, s_off) and np.array_equal(q_idx, s_idx)      # the particles' positions as queries: the SELF rows
    b_off, b_idx, _ = NR.brute_force(pkg, rec["pos"], sp, R, points=pts[:, :3])
    assert np.array_equal(q_off, b_off) and np.array_equal(q_idx, b_idx)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], pts[0, :3]], F)
    off, idx = pkg.neighbors_host(rec, sp, R, points=bad)
    assert off[:4].tolist() == [0, 0, 0, 0] and np.array_equal(idx, s_idx[s_off[0]:s_off[1]])
    far = pts[:5, :3] + F(1e4)                                                 # far outside the grid: clamped cell, nobody in reach
    off, idx = pkg.neighbors_host(rec, sp, R, points=far)
    assert off[-1] == 0 and len(idx) == 0
    c_off, c_idx = pkg.neighbors_host(rec, sp, R, points=pts, count_only=True)
    assert c_idx is None and np.array_equal(c_off, s_off)


def test_argument_errors(pkg):
    rec, sp, _ = _scene(pkg, SEEDS[1])
    L = pkg.load_library()
    h = sp.param_h
    cs = pkg.compute_grid_extents(sp).cellSize
    for bad in (0.0, -h, float("nan"), float("inf"), float(np.nextafter(F(3.0) * F(cs), F(np.inf)))):
        with pytest.raises(pkg.SphError, match="radius"):
            pkg.neighbors_host(rec, sp, bad)
    pkg.neighbors_host(rec, sp, float(F(3.0) * F(cs)))                         # exactly three cells is a radius
    with pytest.raises(pkg.SphError, match="SELF"):
        pkg.neighbors_host(rec, sp, h, self_=True, half=True)
    for kw in (dict(self_=True), dict(half=True)):
        with pytest.raises(pkg.SphError, match="particle lists"):
            pkg.neighbors_host(rec, sp, h, points=rec["pos"][:3], **kw)
    n = len(rec)
    off = np.zeros(n + 1, np.int64)
    idx = np.zeros(4, np.int32)
    info = pkg.SphNeighborInfo()
    args = (rec.ctypes.data_as(C.c_void_p), n, C.byref(sp), None, 0, C.c_float(h))
    assert L.sph_neighbors_host(*args, 8, off.ctypes.data_as(C.c_void_p), None, 0, C.byref(info)) == -1             # unknown flag bit
    assert L.sph_neighbors_host(*args, 0, None, idx.ctypes.data_as(C.c_void_p), 4, C.byref(info)) == -1            # null offsets
    assert L.sph_neighbors_host(*args, 0, off.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 4, None) == -1   # null info
    assert L.sph_neighbors_host(None, n, C.byref(sp), None, 0, C.c_float(h), 0, off.ctypes.data_as(C.c_void_p), None, 0, C.byref(info)) == -1
    # a short index array: SPH_ERR_CAPACITY, the info filled and the offsets valid
    rc = L.sph_neighbors_host(*args, 0, off.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 4, C.byref(info))
    want, _ = pkg.neighbors_host(rec, sp, h)
    assert rc == -4 and info.total == want[-1] > 4 and np.array_equal(off, want) and (idx == 0).all()
    assert (info.rows, info.kind, info.stencil, info.flags) == (n, 1, 1, 0) and info.maxCount == np.diff(want).max()


def test_info_of_every_radius_class(pkg):
    rec, sp, _ = _scene(pkg, SEEDS[0])
    L = pkg.load_library()
    h = sp.param_h
    off = np.zeros(len(rec) + 1, np.int64)
    for R, s in ((0.5 * h, 1), (h, 1), (float(np.nextafter(F(h), F(np.inf))), 2), (2 * h, 2), (2.5 * h, 3), (3 * h, 3)):
        info = pkg.SphNeighborInfo()
        rc = L.sph_neighbors_host(rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(sp), None, 0, C.c_float(R), pkg.SPH_NEIGHBORS_COUNT_ONLY,
                                  off.ctypes.data_as(C.c_void_p), None, 0, C.byref(info))
        assert rc == 0 and info.stencil == s and info.radius == F(R) and info.flags == 4 and info.total == off[-1]


def test_neighbor_info_layout(pkg, tmp_path):
    size, offsets, extra = support.c_layout("SphNeighborInfo", pkg.SphNeighborInfo, [
        'printf("%d %d %d\\n", SPH_NEIGHBORS_SELF, SPH_NEIGHBORS_HALF, SPH_NEIGHBORS_COUNT_ONLY);'], tmp_path)
    assert size == C.sizeof(pkg.SphNeighborInfo) == 40
    assert offsets == [(name, getattr(pkg.SphNeighborInfo, name).offset) for name, _ in pkg.SphNeighborInfo._fields_]
    assert extra == [f"{pkg.SPH_NEIGHBORS_SELF} {pkg.SPH_NEIGHBORS_HALF} {pkg.SPH_NEIGHBORS_COUNT_ONLY}"]
