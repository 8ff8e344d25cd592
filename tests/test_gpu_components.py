"""Connected components on the device (sph_components.h) against sph_components_host byte for byte (labels, roots, table, info except
rounds) on the scenes of components_scenes.py, against the restatement where the margin allows, against the engine's own neighbour
lists, on states the engine produced, and the interface around them."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import components_ref as CR
import components_scenes as CS
from support import after_dispatches, build_example, linked_list_grid, run_example, same_info, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu
F = np.float32
vp = C.c_void_p
INFO_FIELDS = ("rows", "numComponents", "numExcluded", "largestCount", "largestRoot", "numSingletons", "radius", "stencil", "flags")
ROUND_CAP = 64


def _same(pkg, f, rec, sp, R, fluid_only=False, what=""):
    """The engine's result is the host twin's, byte for byte; returns (labels, roots, table, info of the engine)."""
    wl, wr, wt, winfo = pkg.components_host(rec, sp, R, fluid_only=fluid_only)
    labels, roots, table = f.components(R, fluid_only=fluid_only)
    info = f.component_info()
    print(what, "n", len(rec), "bodies", info.numComponents, "largest", info.largestCount, "rounds", info.rounds)
    assert labels.dtype == np.int32 and roots.dtype == np.int32 and table.dtype == pkg.COMPONENT_DTYPE
    assert labels.tobytes() == wl.tobytes(), f"{what}: labels differ"
    assert roots.tobytes() == wr.tobytes(), f"{what}: roots differ"
    assert table.tobytes() == wt.tobytes(), f"{what}: tables differ"
    same_info(info, winfo, INFO_FIELDS, what)
    assert (1 <= info.rounds < ROUND_CAP) if len(rec) else info.rounds == 0
    return labels, roots, table, info


def _all_scenes(pkg):
    return list(CS.scenes(pkg)) + [(name, CS.rec_of(pkg, pos), sp, R, bodies) for name, pos, sp, R, bodies in CS.chain_scenes(pkg)]


def test_scenes(pkg):
    """Sizes 0, 1, 2; threshold pairs in one cell, adjacent cells and at the stencil's outer ring; crowded cells joined and apart;
    interleaved bodies; clamped cells; non-finite records; the ghost bridge; the serpentine chain whole and cut."""
    for name, rec, sp, R, bodies in _all_scenes(pkg):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        labels, roots, table, info = _same(pkg, f, rec, sp, R, what=name)
        assert info.numComponents == bodies, name
        wl, wr, wt, margin = CR.components(pkg, rec, sp, R)
        if margin > 1e-6:
            assert np.array_equal(labels, wl) and np.array_equal(roots, wr), name
            CR.assert_table(table, wt, name)
        if name == "ghost bridge":
            labels, roots, table, info = _same(pkg, f, rec, sp, R, fluid_only=True, what=name + ", fluid only")
            assert labels.tolist() == [0, -1, 1, 0, 1] and (info.numComponents, info.numExcluded) == (2, 1)
        if name == "non-finite":
            assert table["flags"].tolist().count(pkg.SPH_COMPONENT_NONFINITE) == 2 and table["flags"][labels[7]] == 1
        f.close()


def test_chain_orders(pkg):
    """The chain with ids in order, reversed and randomly permuted: one body within the round cap, the host twin's bytes, one table."""
    name, pos, sp, R, _ = next(CS.chain_scenes(pkg))
    tables = []
    for order in (np.arange(len(pos)), np.arange(len(pos))[::-1], np.random.default_rng(0).permutation(len(pos))):
        rec = CS.rec_of(pkg, pos[order])
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        labels, roots, table, info = _same(pkg, f, rec, sp, R, what=name)
        assert info.numComponents == 1 and info.largestCount == len(pos) and not labels.any()
        tables.append(table.tobytes())
        f.close()
    assert tables[0] == tables[1] == tables[2]


@pytest.mark.parametrize("seed", range(12))
def test_random_clouds(pkg, seed):
    """Both sides of percolation: the host twin's bytes, the restatement's bodies, every edge of the engine's own lists inside one body,
    and the same bytes from the two A/B variants of the kernels."""
    import torch
    sp = CS.params(pkg)
    rec, R = CS.cloud(pkg, sp, seed)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    labels, roots, table, info = _same(pkg, f, rec, sp, R, what=f"cloud {seed}")
    wl, wr, wt, margin = CR.components(pkg, rec, sp, R)
    assert margin > 1e-6, "fixture condition: a pair sits on the sphere within rounding"
    assert info.numComponents == len(wt["root"]) and np.array_equal(labels, wl) and np.array_equal(roots, wr)
    CR.assert_table(table, wt)
    g = f.radius_graph(R)
    d_labels, d_roots, d_table = f.components(R, device=True)
    assert d_labels.is_cuda and d_labels.dtype == torch.int32 and d_roots.is_cuda and d_roots.dtype == torch.int32
    assert np.array_equal(d_labels.cpu().numpy(), labels) and np.array_equal(d_roots.cpu().numpy(), roots) and d_table.tobytes() == table.tobytes()
    assert bool((d_labels[g[0]] == d_labels[g[1]]).all()) and g.shape[1] > 0
    for variant in (1, 2, 3):
        f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, variant)
        _same(pkg, f, rec, sp, R, what=f"cloud {seed} variant {variant}")
    f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, 0)
    _same(pkg, f, rec, sp, R, fluid_only=True, what=f"cloud {seed} fluid only")
    f.close()


@pytest.mark.parametrize("kern,aos,graph", [(3, 1, 0), (2, 1, 0), (1, 1, 0), (3, 0, 0), (3, 1, 1), (3, 0, 1)])
def test_after_dispatches(pkg, kern, aos, graph):
    """On a state the engine produced: the components of the downloaded records, twice the same bytes, still there after a dispatch."""
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    rec["isGhost"][::37] = 1

    def check(f, now, sp, what):
        for fac, fluid_only in ((0.6, False), (1.0, True), (2.0, False)):
            R = float(F(fac) * F(sp.param_h))
            first = _same(pkg, f, now, sp, R, fluid_only=fluid_only, what=f"{what} R {fac} h")
            again = f.components(R, fluid_only=fluid_only)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again))
        return first

    def unchanged(f, first):                                                       # the result describes the state it was built from
        info = f.component_info()
        assert info.numComponents == first[3].numComponents
        L = pkg.load_library()
        lab = np.zeros(len(rec), np.int32)
        assert L.sph_components_download(f._h, lab.ctypes.data_as(vp), None, None, 0) == 0 and lab.tobytes() == first[0].tobytes()

    after_dispatches(pkg, kern, aos, graph, check, unchanged, scene=(rec, sp))


def test_components_do_not_change_the_simulation(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)

    def probe(f):
        f.components(0.7 * sp.param_h, fluid_only=True)

    for aos in (1, 0):
        for graph in (0, 1):
            a_up, a, la = undisturbed_run(pkg, rec, sp, probe, aos, graph)
            b_up, b, lb = undisturbed_run(pkg, rec, sp, None, aos, graph)
            assert_records_equal(a_up, b_up, f"upload / download, aos {aos} graph {graph}")
            assert_records_equal(a, b, f"aos {aos} graph {graph}")
            if graph:
                assert la > 0 and lb > 0


def test_refusals_and_states(pkg):
    L = pkg.load_library()
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    info = pkg.SphComponentInfo()
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_components_build(slab._h, sp.param_h, 0, C.byref(info)) == -3 and b"slab" in L.sph_last_error()
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    n = len(rec)
    labels, roots, table = np.full(n, 9, np.int32), np.full(n, 9, np.int32), np.zeros(n, pkg.COMPONENT_DTYPE)
    a, b, c = vp(), vp(), vp()

    def nothing_held():
        assert L.sph_components_info(f._h, C.byref(info)) == -3
        assert L.sph_components_device(f._h, C.byref(a), C.byref(b), C.byref(c)) == -3
        assert L.sph_components_download(f._h, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), n) == -3
        with pytest.raises(pkg.SphError, match="-3"):
            f.component_info()
    nothing_held()                                                                 # before any build
    with linked_list_grid(pkg, f):
        with pytest.raises(pkg.SphError, match="-3"):
            f.components()
    nothing_held()
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * sp.param_h):
        assert L.sph_components_build(f._h, R, 0, C.byref(info)) == -1
    assert L.sph_components_build(f._h, sp.param_h, 2, C.byref(info)) == -1 and L.sph_components_build(f._h, sp.param_h, 0, None) == -1
    assert L.sph_components_build(None, sp.param_h, 0, C.byref(info)) == -1
    nothing_held()
    want = pkg.components_host(rec, sp, 0.6 * sp.param_h)
    got = f.components(0.6 * sp.param_h)
    bodies = len(got[2])
    assert bodies > 1 and all(x.tobytes() == y.tobytes() for x, y in zip(got, want[:3]))
    assert f.components()[0].tobytes() == pkg.components_host(rec, sp, sp.param_h)[0].tobytes()       # radius None: param_h
    f.components(0.6 * sp.param_h)
    assert L.sph_components_device(f._h, C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value and b.value and c.value
    assert L.sph_components_device(f._h, None, C.byref(b), C.byref(c)) == -1 and L.sph_components_info(f._h, None) == -1
    # a short table: nothing written; an exact one is enough; null pointers are skipped
    assert L.sph_components_download(f._h, labels.ctypes.data_as(vp), roots.ctypes.data_as(vp), table.ctypes.data_as(vp), bodies - 1) == -4
    assert (labels == 9).all() and (roots == 9).all() and not table["count"].any()
    assert L.sph_components_download(f._h, None, roots.ctypes.data_as(vp), table.ctypes.data_as(vp), bodies) == 0
    assert (labels == 9).all() and roots.tobytes() == want[1].tobytes() and table[:bodies].tobytes() == want[2].tobytes() and not table["count"][bodies:].any()
    # the option
    assert f.get_option(pkg.SPH_OPT_COMPONENTS_VARIANT) == 0
    for bad in (-1, 4):
        with pytest.raises(pkg.SphError):
            f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, bad)
    # valid after a dispatch, ended by a reset
    f.DispatchN(2)
    assert f.component_info().numComponents == bodies
    f.ResetSimulation()
    nothing_held()
    f.close()


def test_droplets_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "droplets", tmp_path, werror=True), ["20000", "3"], timeout=120)
    assert res.returncode == 0 and "droplets OK" in res.stdout
    assert len([ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]) == 3
