"""k nearest neighbours on the CPU (sph_knn_host: the kernels' r2 and key over the counting sort of sph_neighbors_host) against the float64
restatement of knn_ref.py, the bit-level consequences of the definition (prefix rows, the neighbour lists' sets, exact ties), the flags,
query rows, argument errors and the layout of SphKnnInfo.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import knn_ref as KR
import neighbors_ref as NR
import query_scenes as QS
import support

F = np.float32
vp = C.c_void_p
# (particles, k, R) in the 4 x 3 x 3.5 box at h = 0.5: R = 2h, h, 3h; k = 64 only at R <= 1.0 with 2000 particles (about 140 candidates a row)
SHAPES = ((2000, 16, 1.0), (2000, 8, 0.5), (4000, 32, 1.5), (2000, 64, 1.0))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _rows(idx, cnt):
    return [idx[i, :cnt[i]] for i in range(len(cnt))]


def _well_formed(idx, d2, cnt, k, n):
    """What every result satisfies: shapes, padding, index range, ascending (dist2, id)."""
    assert idx.shape == d2.shape == (len(cnt), k) and idx.dtype == np.int32 and d2.dtype == F and cnt.dtype == np.uint32
    col = np.arange(k)[None, :]
    pad = col >= cnt[:, None]
    assert (cnt <= k).all() and (idx[pad] == -1).all() and np.isposinf(d2[pad]).all()
    assert ((idx[~pad] >= 0) & (idx[~pad] < max(n, 1))).all() and np.isfinite(d2[~pad]).all() and (d2[~pad] >= 0).all()
    key = (_bits(d2).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32).astype(np.uint64)
    both = ~pad[:, 1:]
    assert (key[:, 1:][both] > key[:, :-1][both]).all(), "a row is not strictly ascending in (dist2, id)"


@pytest.mark.parametrize("n,k,R", SHAPES)
def test_host_equals_the_float64_restatement(pkg, n, k, R):
    """Near-tie rows at 1e-6 R^2 (the threshold the comparison uses), measured on these seeded scenes: 2000 / k 16 / R 1.0: 0.15 %;
    2000 / k 8 / R 0.5: 0 %; 4000 / k 32 / R 1.5: 1.00 %; 2000 / k 64 / R 1.0: 0.40 % (printed below; the bound of 5 % is a condition on
    the inputs, checked on the restatement alone before anything is compared)."""
    rec, sp = QS.uniform(pkg, n, seed=n + k)
    assert NR.inside_grid(pkg, rec["pos"], sp)
    w_idx, w_d2, w_cnt, near, edge = KR.knn(rec["pos"], k, R)
    share = near.mean()
    assert not edge.any(), "fixture condition: a rejected candidate sits on the sphere within rounding"
    print(f"n {n} k {k} R {R}: near-tie rows {100 * share:.2f} %, full rows {(w_cnt == k).mean():.2f}, mean count {w_cnt.mean():.1f}")
    assert share <= 0.05, "fixture condition: too many near-tie rows"
    idx, d2, cnt, info = pkg.knn_host(rec, sp, k, R)
    _well_formed(idx, d2, cnt, k, n)
    tol = 1e-6 * R * R
    assert np.array_equal(cnt.astype(np.int64), w_cnt)
    firm = ~near
    assert np.array_equal(idx[firm], w_idx[firm])
    fin = np.isfinite(w_d2)
    assert np.array_equal(np.isfinite(d2), fin) and (np.abs(d2.astype(np.float64)[fin] - w_d2[fin]) <= tol).all()     # (rows are sorted: also on the near-tie rows)
    assert (info.rows, info.total, info.rowsFull, info.k, info.kind, info.flags) == (n, w_cnt.sum(), (w_cnt == k).sum(), k, 1, 0)
    assert info.radius == F(R) and info.stencil == int(np.ceil(R / sp.param_h))


def test_prefix_property(pkg):
    rec, sp = QS.uniform(pkg, 2000, seed=21)
    ks = (1, 7, 8, 9, 16, 33, 64)
    res = {k: pkg.knn_host(rec, sp, k, 1.0) for k in ks}
    i64, d64, c64, _ = res[64]
    for k in ks:
        idx, d2, cnt, _ = res[k]
        _well_formed(idx, d2, cnt, k, len(rec))
        assert np.array_equal(cnt, np.minimum(c64, k))
        keep = np.arange(k)[None, :] < cnt[:, None]
        assert np.array_equal(idx[keep], i64[:, :k][keep]) and np.array_equal(_bits(d2)[keep], _bits(d64)[:, :k][keep])
    assert (c64 == 64).any() and (c64 < 64).any()


@pytest.mark.parametrize("self_", [False, True])
def test_rows_are_the_neighbour_lists_when_k_covers_them(pkg, self_):
    rec, sp = QS.uniform(pkg, 2000, seed=22)
    n = len(rec)
    for R, k in ((0.5, 64), (1.0, 8), (1.3, 17)):
        off, nidx = pkg.neighbors_host(rec, sp, R, self_=self_)
        deg = np.diff(off)
        idx, d2, cnt, info = pkg.knn_host(rec, sp, k, R, self_=self_)
        assert np.array_equal(cnt.astype(np.int64), np.minimum(deg, k)) and info.total == np.minimum(deg, k).sum()
        covered = np.flatnonzero(deg <= k)
        assert R != 0.5 or len(covered) == n                                     # (at R = h every row is shorter than 64)
        for i in covered:
            assert np.array_equal(np.sort(idx[i, :cnt[i]]), np.sort(nidx[off[i]:off[i + 1]])), i
        if self_:
            assert (idx[:, 0] == np.arange(n)).all() and (d2[:, 0] == 0).all()      # (no two particles of this cloud coincide)
        else:
            assert not (idx == np.arange(n)[:, None]).any()
    assert pkg.neighbors_host(rec, sp, 0.5)[0][-1] > 0 and np.diff(pkg.neighbors_host(rec, sp, 0.5)[0]).max() <= 64


def test_exact_ties_on_a_lattice_resolve_by_id(pkg):
    """Spacing h / 2 with exactly representable coordinates: every r2 is exact in fp32 and in float64, whole shells tie, and the order
    inside a shell is the id order -- the restatement's rows, entry for entry, although every row is a (near-)tie row."""
    rec, sp = QS.lattice(pkg)
    for k, R in ((6, 0.5), (7, 0.5), (19, 1.0), (64, 1.0)):
        w_idx, w_d2, w_cnt, near, edge = KR.knn(rec["pos"], k, R)
        idx, d2, cnt, _ = pkg.knn_host(rec, sp, k, R)
        assert near.mean() > 0.9                                                  # (edge: lattice points at exactly R are rejected exactly on both sides)
        assert np.array_equal(idx, w_idx) and np.array_equal(cnt.astype(np.int64), w_cnt) and np.array_equal(d2.astype(np.float64), w_d2)
        tied = d2[:, 1:] == d2[:, :-1]
        assert tied.any() and (idx[:, 1:][tied & np.isfinite(d2[:, 1:])] > idx[:, :-1][tied & np.isfinite(d2[:, 1:])]).all()


def test_coincident_particles_are_ordered_by_id(pkg):
    rec, sp, same = QS.coincident(pkg)
    for k in (4, 8, 16):
        idx, d2, cnt, _ = pkg.knn_host(rec, sp, k, 1.0, self_=True)
        for i in same:
            assert idx[i, :min(k, 8)].tolist() == same[:min(k, 8)].tolist() and (d2[i, :min(k, 8)] == 0).all()
            assert k <= 8 or d2[i, 8] > 0
        idx, d2, cnt, _ = pkg.knn_host(rec, sp, k, 1.0)
        for i in same:
            others = same[same != i]
            assert idx[i, :min(k, 7)].tolist() == others[:min(k, 7)].tolist() and (d2[i, :min(k, 7)] == 0).all()
    # as query points: the SELF rows
    q = pkg.knn_host(rec, sp, 16, 1.0, points=rec["pos"][:, :3])
    s = pkg.knn_host(rec, sp, 16, 1.0, self_=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(q[:3], s[:3]))


def test_fluid_only_with_ghosts_of_every_kind(pkg):
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    assert set(np.unique(rec["isGhost"])) == {0, 1, 3} and (rec["isActive"] == 0).any()
    for k, R in ((8, 1.0), (33, 1.5)):
        idx, d2, cnt, info = pkg.knn_host(rec, sp, k, R, fluid_only=True)
        _well_formed(idx, d2, cnt, k, len(rec))
        assert (cnt[ghost] == 0).all() and (cnt[~ghost] > 0).all() and not ghost[idx[idx >= 0]].any() and info.flags == pkg.SPH_KNN_FLUID_ONLY
        w_idx, w_d2, w_cnt, near, edge = KR.knn(rec["pos"], k, R, exclude=ghost)
        assert near.mean() <= 0.05 and not edge.any() and np.array_equal(cnt.astype(np.int64), w_cnt) and np.array_equal(idx[~near], w_idx[~near])
        # without the flag ghosts and inactive records are records like any other
        a_idx, _, a_cnt, _ = pkg.knn_host(rec, sp, k, R)
        assert ghost[a_idx[a_idx >= 0]].any() and (a_cnt[ghost] > 0).all()
        # query rows may be fluid-only too
        q_idx, _, q_cnt, _ = pkg.knn_host(rec, sp, k, R, points=rec["pos"][:50, :3], fluid_only=True)
        assert not ghost[q_idx[q_idx >= 0]].any() and (q_cnt > 0).all()


def test_non_finite_particles_and_query_points(pkg):
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    for self_ in (False, True):
        idx, d2, cnt, _ = pkg.knn_host(rec, sp, 16, 1.0, self_=self_)
        assert cnt[7] == 0 and cnt[300] == 0 and not np.isin(idx, (7, 300)).any()     # SELF is an ordinary candidate: r2 is NaN
        assert (idx[7] == -1).all() and np.isposinf(d2[300]).all()
    pts = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], rec["pos"][0, :3], rec["pos"][0, :3] + F(1e4)], F)
    idx, d2, cnt, info = pkg.knn_host(rec, sp, 5, 1.0, points=pts)
    assert cnt.tolist()[:3] == [0, 0, 0] and cnt[3] == 5 and cnt[4] == 0 and idx[3, 0] == 0 and d2[3, 0] == 0
    assert (info.rows, info.kind, info.total, info.rowsFull) == (5, 2, 5, 1)


def test_argument_refusals(pkg):
    rec, sp = QS.uniform(pkg, 200, seed=24)
    L = pkg.load_library()
    h = sp.param_h
    cs = pkg.compute_grid_extents(sp).cellSize
    for bad in (0.0, -h, float("nan"), float("inf"), float(np.nextafter(F(3.0) * F(cs), F(np.inf)))):
        with pytest.raises(pkg.SphError, match="radius"):
            pkg.knn_host(rec, sp, 8, bad)
    pkg.knn_host(rec, sp, 8, float(F(3.0) * F(cs)))                               # exactly three cells is a radius
    for bad in (0, -1, 65, 1 << 20):
        with pytest.raises(pkg.SphError, match="k = "):
            pkg.knn_host(rec, sp, bad, h)
    with pytest.raises(pkg.SphError, match="particle rows"):
        pkg.knn_host(rec, sp, 8, h, points=rec["pos"][:3], self_=True)
    n = len(rec)
    info = pkg.SphKnnInfo()
    idx, d2, cnt = np.zeros((n, 8), np.int32), np.zeros((n, 8), F), np.zeros(n, np.uint32)
    out = (idx.ctypes.data_as(vp), d2.ctypes.data_as(vp), cnt.ctypes.data_as(vp))
    args = (rec.ctypes.data_as(vp), n, C.byref(sp), None, 0, 8, C.c_float(h))
    assert L.sph_knn_host(*args, 4, *out, C.byref(info)) == -1                     # unknown flag bit
    assert L.sph_knn_host(*args, 0, *out, None) == -1                              # null info
    assert L.sph_knn_host(None, n, C.byref(sp), None, 0, 8, C.c_float(h), 0, *out, C.byref(info)) == -1
    assert L.sph_knn_host(rec.ctypes.data_as(vp), n, None, None, 0, 8, C.c_float(h), 0, *out, C.byref(info)) == -1
    assert not idx.any() and not cnt.any()
    assert L.sph_knn_host(*args, 0, None, None, cnt.ctypes.data_as(vp), C.byref(info)) == 0      # any output may be null
    assert info.total == cnt.sum() and np.array_equal(cnt, pkg.knn_host(rec, sp, 8, h)[2])


def test_tiny_inputs(pkg):
    sp = QS.params(pkg)
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    idx, d2, cnt, info = pkg.knn_host(none, sp, 8, 1.0)
    assert idx.shape == (0, 8) and cnt.shape == (0,) and (info.rows, info.total, info.rowsFull, info.kind) == (0, 0, 0, 1)
    idx, d2, cnt, info = pkg.knn_host(none, sp, 8, 1.0, points=np.zeros((3, 3), F))
    assert (idx == -1).all() and np.isposinf(d2).all() and cnt.tolist() == [0, 0, 0] and (info.rows, info.kind) == (3, 2)
    one = support.records(pkg, np.array([[0.2, -0.4, 0.1]], F), np.zeros((1, 3), F))
    idx, d2, cnt, info = pkg.knn_host(one, sp, 4, 1.0)
    assert idx.tolist() == [[-1] * 4] and cnt.tolist() == [0]
    idx, d2, cnt, info = pkg.knn_host(one, sp, 4, 1.0, self_=True)
    assert idx.tolist() == [[0, -1, -1, -1]] and d2[0, 0] == 0 and cnt.tolist() == [1] and info.rowsFull == 0
    idx, d2, cnt, info = pkg.knn_host(one, sp, 4, 1.0, points=np.zeros((0, 3), F))
    assert idx.shape == (0, 4) and (info.rows, info.kind) == (0, 2)
    # k > n: every row shorter than k
    rec, sp = QS.uniform(pkg, 20, seed=25)
    idx, d2, cnt, info = pkg.knn_host(rec, sp, 64, 1.5)
    _well_formed(idx, d2, cnt, 64, 20)
    assert (cnt < 20).all() and info.rowsFull == 0 and cnt.sum() == info.total > 0


def test_knn_info_layout(pkg, tmp_path):
    size, offsets, extra = support.c_layout("SphKnnInfo", pkg.SphKnnInfo, [
        'printf("%d %d %d %d\\n", SPH_KNN_SELF, SPH_KNN_FLUID_ONLY, SPH_KNN_MAX_K, SPH_OPT_KNN_VARIANT);'], tmp_path)
    assert size == C.sizeof(pkg.SphKnnInfo) == 48
    assert offsets == [(name, getattr(pkg.SphKnnInfo, name).offset) for name, _ in pkg.SphKnnInfo._fields_]
    assert extra == [f"{pkg.SPH_KNN_SELF} {pkg.SPH_KNN_FLUID_ONLY} {pkg.SPH_KNN_MAX_K} {pkg.SPH_OPT_KNN_VARIANT}"]
