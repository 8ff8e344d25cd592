"""Connected components on the CPU (sph_components_host: a sequential union-find over the counting sort of sph_neighbors_host) against
the restatement of components_ref.py, on the scenes of components_scenes.py; the numbering rules, SPH_COMPONENTS_FLUID_ONLY, argument
errors, the fixed-point sums and the layout of the two records.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import components_ref as CR
import components_scenes as CS
import support

F = np.float32
SCENES = None


def _scenes(pkg):
    global SCENES
    if SCENES is None:
        SCENES = list(CS.scenes(pkg)) + [(name, CS.rec_of(pkg, pos), sp, R, bodies) for name, pos, sp, R, bodies in CS.chain_scenes(pkg)]
    return SCENES


def _check_rules(pkg, rec, labels, roots, table, info, fluid_only=False):
    """What holds for every result, whatever the scene: the canonical names and the books of the table and the info."""
    n = len(rec)
    part = np.ones(n, bool) if not fluid_only else rec["isGhost"] == 0
    assert labels.dtype == np.int32 and roots.dtype == np.int32 and len(labels) == len(roots) == n
    assert (labels[~part] == -1).all() and (roots[~part] == -1).all()
    C_ = len(table)
    assert ((labels[part] >= 0) & (labels[part] < C_)).all()
    assert np.array_equal(np.bincount(labels[part], minlength=C_), table["count"]) and int(table["count"].sum()) == int(part.sum())
    assert (np.diff(table["root"].astype(np.int64)) > 0).all()                          # numbered in ascending order of the smallest id
    for c in range(C_):
        m = np.flatnonzero(labels == c)
        assert m[0] == table["root"][c] and (roots[m] == m[0]).all()
    want = CR.info_of(labels, roots, table)
    assert {k: int(getattr(info, k)) for k in want} == want


@pytest.mark.parametrize("index", range(28))
def test_host_components_on_the_scenes(pkg, index):
    scenes = _scenes(pkg)
    assert len(scenes) == 28
    name, rec, sp, R, bodies = scenes[index]
    labels, roots, table, info = pkg.components_host(rec, sp, R)
    print(name, "n", len(rec), "bodies", info.numComponents, "largest", info.largestCount)
    assert info.numComponents == len(table) == bodies, name
    _check_rules(pkg, rec, labels, roots, table, info)
    wl, wr, wt, margin = CR.components(pkg, rec, sp, R)
    if margin > 1e-6:                                                                   # (the threshold scenes sit on the sphere on purpose)
        assert np.array_equal(labels, wl) and np.array_equal(roots, wr), name
        CR.assert_table(table, wt, name)
    else:
        assert "threshold" in name or "combs" in name, f"{name}: margin {margin}"


@pytest.mark.parametrize("seed", range(12))
def test_host_components_of_random_clouds(pkg, seed):
    sp = CS.params(pkg)
    rec, R = CS.cloud(pkg, sp, seed)
    labels, roots, table, info = pkg.components_host(rec, sp, R)
    wl, wr, wt, margin = CR.components(pkg, rec, sp, R)
    print("seed", seed, "n", len(rec), "R", R, "bodies", info.numComponents, "largest", info.largestCount, "singletons", info.numSingletons, "margin", margin)
    assert margin > 1e-6, "fixture condition: a pair sits on the sphere within rounding"
    assert np.array_equal(labels, wl) and np.array_equal(roots, wr)
    CR.assert_table(table, wt)
    _check_rules(pkg, rec, labels, roots, table, info)
    assert (info.radius, info.flags, info.rounds) == (F(R), 0, 0) and info.stencil == int(np.ceil(F(R) / F(sp.param_h)))


def test_chain_orders_give_the_same_table(pkg):
    """Ids along the chain, reversed and randomly permuted: one body, and a table that does not depend on the numbering."""
    name, pos, sp, R, _ = next(CS.chain_scenes(pkg))
    tables = []
    for order in (np.arange(len(pos)), np.arange(len(pos))[::-1], np.random.default_rng(0).permutation(len(pos))):
        labels, roots, table, info = pkg.components_host(CS.rec_of(pkg, pos[order]), sp, R)
        assert info.numComponents == 1 and info.largestCount == len(pos) and not labels.any() and not roots.any()
        tables.append(table.tobytes())
    assert tables[0] == tables[1] == tables[2]


def test_fluid_only_and_the_ghost_bridge(pkg):
    name, rec, sp, R, _ = [s for s in _scenes(pkg) if s[0] == "ghost bridge"][0]
    labels, roots, table, info = pkg.components_host(rec, sp, R)
    assert info.numComponents == 1 and info.numExcluded == 0 and table["count"].tolist() == [5]
    labels, roots, table, info = pkg.components_host(rec, sp, R, fluid_only=True)
    assert labels.tolist() == [0, -1, 1, 0, 1] and roots.tolist() == [0, -1, 2, 0, 2]
    assert (info.numComponents, info.numExcluded, info.flags) == (2, 1, pkg.SPH_COMPONENTS_FLUID_ONLY)
    _check_rules(pkg, rec, labels, roots, table, info, fluid_only=True)
    wl, wr, wt, margin = CR.components(pkg, rec, sp, R, fluid_only=True)
    assert margin > 1e-6 and np.array_equal(labels, wl) and np.array_equal(roots, wr)
    CR.assert_table(table, wt)
    # ghosts only: nothing takes part
    rec["isGhost"] = 3
    labels, roots, table, info = pkg.components_host(rec, sp, R, fluid_only=True)
    assert (labels == -1).all() and (roots == -1).all() and len(table) == 0 and (info.numComponents, info.numExcluded, info.largestCount) == (0, 5, 0)


def test_non_finite_records_and_the_fixed_point_sums(pkg):
    name, rec, sp, R, _ = [s for s in _scenes(pkg) if s[0] == "non-finite"][0]
    labels, roots, table, info = pkg.components_host(rec, sp, R)
    for i in (7, 30):
        row = table[labels[i]]
        assert row["flags"] == pkg.SPH_COMPONENT_NONFINITE and row["count"] == 1 and row["root"] == i
        assert not row["bbMin"].any() and not row["bbMax"].any() and not row["sumQ"].any()
    big = table[labels[0]]
    assert big["count"] == 38 and big["flags"] == 0
    q = CR.fixed_point(pkg, rec["pos"], sp)
    members = np.flatnonzero(labels == labels[0])
    assert big["sumQ"].tolist() == q[members].sum(axis=0).tolist()
    # the centre from the sums is the mean position to within the resolution of the fixed point (cellSize / 65536 per record)
    g = pkg.compute_grid_extents(sp)
    ctr = pkg.component_centers(table, g)
    mean = rec["pos"][members, :3].astype(np.float64).mean(axis=0)
    assert np.abs(ctr[labels[0]] - mean).max() <= 0.5 * g.cellSize / 65536.0 + 1e-12
    assert np.isnan(ctr[labels[7]]).all()
    # a position far outside clamps at +-2^36
    far = CS.rec_of(pkg, [[3.0e30, -3.0e30, 0.0]])
    _, _, t, _ = pkg.components_host(far, sp, R)
    assert t["sumQ"][0, 0] == 2 ** 36 and t["sumQ"][0, 1] == -2 ** 36 and t["bbMin"][0, 0] == F(3.0e30)


def test_argument_errors(pkg):
    name, rec, sp, R, _ = _scenes(pkg)[10]
    L = pkg.load_library()
    h = sp.param_h
    cs = pkg.compute_grid_extents(sp).cellSize
    for bad in (0.0, -h, float("nan"), float("inf"), float(np.nextafter(F(3.0) * F(cs), F(np.inf)))):
        with pytest.raises(pkg.SphError, match="radius"):
            pkg.components_host(rec, sp, bad)
    pkg.components_host(rec, sp, float(F(3.0) * F(cs)))                                # exactly three cells is a radius
    n = len(rec)
    labels, roots, table = np.full(n, 9, np.int32), np.full(n, 9, np.int32), np.zeros(n, pkg.COMPONENT_DTYPE)
    info = pkg.SphComponentInfo()
    vp = C.c_void_p
    args = (rec.ctypes.data_as(vp), n, C.byref(sp), C.c_float(h))
    assert L.sph_components_host(*args, 2, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), n, C.byref(info)) == -1
    assert L.sph_components_host(*args, 0, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), n, None) == -1
    assert L.sph_components_host(None, n, C.byref(sp), C.c_float(h), 0, None, None, None, 0, C.byref(info)) == -1
    # a short table: SPH_ERR_CAPACITY, nothing written but the info
    want = pkg.components_host(rec, sp, h)
    bodies = len(want[2])
    assert bodies > 1
    rc = L.sph_components_host(*args, 0, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), bodies - 1, C.byref(info))
    assert rc == -4 and info.numComponents == bodies and (labels == 9).all() and (roots == 9).all() and not table["count"].any()
    # null outputs are skipped
    assert L.sph_components_host(*args, 0, None, None, None, 0, C.byref(info)) == 0 and info.numComponents == bodies
    assert L.sph_components_host(*args, 0, labels.ctypes.data_as(vp), None, table.ctypes.data_as(vp), bodies, C.byref(info)) == 0
    assert np.array_equal(labels, want[0]) and (roots == 9).all() and table[:bodies].tobytes() == want[2].tobytes()


def test_record_layouts(pkg, tmp_path):
    size, offsets, extra = support.c_layout("SphComponent", pkg.SphComponent, [
        'printf("%d %d\\n", SPH_COMPONENTS_FLUID_ONLY, SPH_COMPONENT_NONFINITE);'], tmp_path)
    assert size == C.sizeof(pkg.SphComponent) == pkg.COMPONENT_DTYPE.itemsize == 64
    assert offsets == [(name, getattr(pkg.SphComponent, name).offset) for name, _ in pkg.SphComponent._fields_]
    assert extra == [f"{pkg.SPH_COMPONENTS_FLUID_ONLY} {pkg.SPH_COMPONENT_NONFINITE}"]
    size, offsets, _ = support.c_layout("SphComponentInfo", pkg.SphComponentInfo, [], tmp_path)
    assert size == C.sizeof(pkg.SphComponentInfo) == 56
    assert offsets == [(name, getattr(pkg.SphComponentInfo, name).offset) for name, _ in pkg.SphComponentInfo._fields_]
