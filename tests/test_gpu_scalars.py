"""Diffusing scalar channels on the GPU (include/sph_abi.h "diffusing scalar fields").

Every comparison is bitwise and covers every particle.  The device is compared with the host twin sph_scalars_step_host (which
tests/test_scalars_cpu.py pins to the numpy restatement) on the records the engine itself hands out: download, step the twin,
dispatch, compare."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import scalar_ref as R
import stats_ref
from support import G, build_example, engine, fluid_block, records, run_example, same_bits, undisturbed_run

pytestmark = pytest.mark.gpu

F = np.float32
STEPS = 5


def _state(pkg, name):
    if name == "scene4096":
        _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
        return np.load(os.path.join(G, "scene4096.npz"))["after_10"], sp
    if name == "cylinder2000":
        z = np.load(os.path.join(G, "cylinder2000.npz"))
        return z["after"], pkg.default_params(param_shapeType=2, param_boxHalf=(2.2, 1.6, 0.9), param_boxEulerDeg=(10.0, -25.0, 40.0),
                                              param_boxCenter=(0.2, -0.1, 0.3), param_mass=float(z["mass"]))
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    return fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))


def _coefficients(pkg, rec, sp, K):
    """K diffusivities around a diffusion number of 0.4 on this state, K decay rates (channel 0 conserves)."""
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0)
    assert s1 > 0
    return np.linspace(1.0, 0.4, K).astype(F) * F(0.4 / float(s1)), np.linspace(0.0, 2.0, K).astype(F)


def _values(n, K, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, (n, K)).astype(F)


def _scalar_engine(pkg, rec, sp, c, D, lam, kern=3, aos=1, graph=0, staged=0):
    f = engine(pkg, rec, sp, kern, aos, graph)
    f.set_option(pkg.SPH_OPT_SCALAR_SWEEP, staged)
    f.set_scalars(c, diffusivity=D, decay=lam)
    return f


_REFERENCE = {}


def _reference(pkg, name, K):
    """(records, params, initial values, D, lambda, [twin values after substep 1 .. STEPS], [twin numbers]), once per state and K:
    the twin steps on the records an engine downloads before each of its substeps."""
    if (name, K) not in _REFERENCE:
        rec, sp = _state(pkg, name)
        D, lam = _coefficients(pkg, rec, sp, K)
        c = _values(len(rec), K)
        f = engine(pkg, rec, sp)
        want, numbers, cur = [], [], c
        for _ in range(STEPS):
            cur, s = pkg.scalars_step_host(f.download(), sp, cur, diffusivity=D, decay=lam)
            f.DispatchCompute()
            want.append(cur)
            numbers.append(s)
        f.close()
        _REFERENCE[(name, K)] = (rec, sp, c, D, lam, want, numbers)
    return _REFERENCE[(name, K)]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", ["scene4096", "cylinder2000", "settled_pool"])
def test_device_equals_the_host_twin(pkg, name, K):
    rec, sp, c, D, lam, want, numbers = _reference(pkg, name, K)
    assert (want[0] != c).any() and (want[-1] != want[0]).any()
    for staged in (0, 1):
        for kern in (3, 2, 1):
            for aos in (0, 1):
                what = f"{name} K={K} staged={staged} pass {kern} aos {aos}"
                f = _scalar_engine(pkg, rec, sp, c, D, lam, kern, aos, staged=staged)
                assert f.num_scalar_channels() == K and f.scalar_info() == (0, 0)
                f.DispatchCompute()
                same_bits(f.scalars(), want[0], what + " after 1 substep")
                assert f.scalar_info()[1].tobytes() == F(numbers[0]).tobytes(), what
                for _ in range(STEPS - 1):
                    f.DispatchCompute()
                same_bits(f.scalars(), want[-1], what + f" after {STEPS} substeps")
                steps, number = f.scalar_info()
                assert steps == STEPS and number.tobytes() == F(numbers[-1]).tobytes(), what
                f.close()


@pytest.mark.parametrize("staged", [0, 1])
def test_graph_replay_equals_eager_dispatch(pkg, staged):
    rec, sp, c, D, lam, _, _ = _reference(pkg, "scene4096", 4)
    e = _scalar_engine(pkg, rec, sp, c, D, lam, staged=staged)
    for _ in range(5):                                                   # (an even count: the state buffers are the same at every call)
        e.DispatchN(4)
    want, want_rec, want_info = e.scalars(), e.download(), e.scalar_info()
    e.close()
    g = _scalar_engine(pkg, rec, sp, c, D, lam, graph=1, staged=staged)
    for _ in range(5):
        g.DispatchN(4)
    assert g.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) >= 2                # captured once, then replayed
    same_bits(g.scalars(), want, "graph replay")
    assert_records_equal(g.download(), want_rec, "records under graph replay")
    assert g.scalar_info() == want_info and want_info[0] == 20
    # coefficients changed between two replays take effect, and a call with scalars is never served by a graph captured without them
    launches = g.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
    g.set_scalar_coefficients(diffusivity=D * F(0.5), decay=lam)
    g.DispatchN(4)
    assert g.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches + 1
    e = _scalar_engine(pkg, rec, sp, c, D, lam, staged=staged)
    for _ in range(5):
        e.DispatchN(4)
    e.set_scalar_coefficients(diffusivity=D * F(0.5), decay=lam)
    e.DispatchN(4)
    same_bits(g.scalars(), e.scalars(), "replay after set_scalar_coefficients")
    assert (g.scalars() != want).any()
    e.clear_scalars()
    g.clear_scalars()
    for f in (e, g):
        for _ in range(3):
            f.DispatchN(4)
    assert_records_equal(g.download(), e.download(), "records after the set was dropped")
    assert g.num_scalar_channels() == 0 and g.scalars().shape == (0, 0)
    e.close()
    g.close()


def _crafted(pkg, name):
    """(records, params, K): the smallest shapes at which the sweep can go wrong."""
    sp = pkg.default_params(param_boxHalf=(2.0, 2.0, 2.0), param_boxCenter=(0.0, 0.0, 0.0), param_boxEulerDeg=(0.0, 0.0, 0.0))
    g = pkg.compute_grid_extents(sp)
    lo, h = np.array(list(g.gridMin), F), F(g.cellSize)
    dims = np.array(list(g.dims))
    rng = np.random.default_rng(sum(map(ord, name)))

    def cell(ix, iy, iz, count):
        return (lo + (np.array([ix, iy, iz], F) + rng.uniform(0.02, 0.98, (count, 3)).astype(F)) * h).astype(F)

    K, ghost = 2, None
    mid = dims // 2
    if name.startswith("cell"):
        pos = np.concatenate([cell(*mid, int(name[4:])), cell(mid[0] + 1, mid[1], mid[2], 9), cell(mid[0], mid[1] - 1, mid[2] + 1, 5)])
    elif name == "straddle":                                             # 250 slots, then a cell run across slot 256
        pos = np.concatenate([cell(2, mid[1], mid[2], 250), cell(3, mid[1], mid[2], 20), cell(4, mid[1], mid[2], 30)])
    elif name == "overflow":                                             # more candidates around one block than the LDS stage holds
        pos = np.concatenate([cell(mid[0] + dx, mid[1] + dy, mid[2] + dz, 70) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)])
        K = 4
    elif name == "edges":                                                # edge and corner cells, and points outside the grid (clamped cell)
        far = np.array([[50, 50, 50], [-50, 0, 0], [0, -60, 70], [1e20, 0, 0]], F)
        top = dims - 1
        pos = np.concatenate([cell(0, 0, 0, 12), cell(top[0], top[1], top[2], 12), cell(0, top[1], mid[2], 12), cell(top[0], 0, 0, 7),
                              (lo - F(0.05) * h + np.zeros((3, 3), F)).astype(F), (lo + (dims.astype(F) + F(0.03)) * h + np.zeros((2, 3), F)).astype(F), far])
        pos[-9:-4] += rng.uniform(-0.01, 0.01, (5, 3)).astype(F)         # (distinct points just outside the two corners)
    elif name == "single":
        pos = cell(*mid, 1)
    elif name == "ghosts":
        pos = np.concatenate([cell(*mid, 40), cell(mid[0] + 1, mid[1], mid[2], 40)])
        ghost = np.ones(len(pos), np.int32)
        ghost[::3] = 2
    else:
        raise KeyError(name)
    rec = records(pkg, pos, np.zeros_like(pos), ghost=ghost)
    rec["isActive"] = 1
    return rec, sp, K


@pytest.mark.parametrize("name", ["cell63", "cell64", "cell65", "cell200", "straddle", "overflow", "edges", "single", "ghosts"])
def test_crafted_scenes(pkg, name):
    rec, sp, K = _crafted(pkg, name)
    c = _values(len(rec), K, 21)
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0)
    D = F(0.4 / float(s1)) if s1 > 0 else F(1.0)
    lam = np.linspace(0.0, 1.0, K).astype(F)
    want, number = pkg.scalars_step_host(rec, sp, c, diffusivity=D, decay=lam)
    if name == "ghosts":
        same_bits(want, c, "an engine of ghosts keeps every value")
        assert number == 0
    elif name == "single":
        assert number == 0 and (want[0, 1] != c[0, 1])                   # no pair; the decay of channel 1 still acts
    else:
        assert number > 0 and (want != c).any(axis=1).sum() > len(rec) // 2
    got = []
    for staged in (0, 1):
        f = _scalar_engine(pkg, rec, sp, c, D, lam, staged=staged)
        f.DispatchCompute()
        got.append((f.scalars(), f.scalar_info()))
        f.close()
    same_bits(got[1][0], got[0][0], f"{name}: staged sweep against the plain sweep")
    same_bits(got[0][0], want, f"{name}: plain sweep against the host twin")
    for values, (steps, s) in got:
        assert steps == 1 and s.tobytes() == F(number).tobytes(), name


def _probe(pkg, D):
    def probe(f):
        if f.num_scalar_channels() == 0:
            f.set_scalars(None, diffusivity=(D, D * F(0.5)), decay=(0.0, 1.0), channels=2)
        centre = np.array(f.param_boxCenter, F)
        f.paint_scalar(centre, 1.5, 1.0, channel=1, mode=pkg.SPH_SCALAR_ADD)
        f.scalar_moments()
        f.sample_scalar(np.array([centre, centre + F(0.3)], F), channel=1)
        f.scalar_info()
    return probe


@pytest.mark.parametrize("graph", [0, 1])
def test_simulation_is_untouched(pkg, graph):
    rec, sp, _, D, _, _, _ = _reference(pkg, "scene4096", 1)
    plain = undisturbed_run(pkg, rec, sp, None, aos=1, graph=graph)
    seen = undisturbed_run(pkg, rec, sp, _probe(pkg, D[0]), aos=1, graph=graph)
    assert_records_equal(seen[0], plain[0], "records after the upload, with and without scalars")
    assert_records_equal(seen[1], plain[1], "records at the end, with and without scalars")
    if graph:
        assert seen[2] >= 1                                              # the graph launch counter advanced


def test_paint_set_and_add(pkg):
    rec, sp, _, D, _, _, _ = _reference(pkg, "scene4096", 1)
    rec = rec.copy()
    rec["isGhost"][100:120] = 1
    rec["pos"][0, :3] = (0.25, 0.5, -0.75)                               # exactly on the first sphere: dx = -0.5, dot3 = 0.25 = r * r
    rec["pos"][1, :3] = (0.25 + 2.0 ** -20, 0.5, -0.75)                  # just inside it
    centre, radius = np.array([0.75, 0.5, -0.75], F), F(0.5)

    def inside(pos, centre, radius):
        d = (pos[:, :3].astype(F) - centre).astype(F)
        with np.errstate(all="ignore"):
            return R.dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]) < F(radius * radius)

    c = _values(len(rec), 2, 8)
    f = _scalar_engine(pkg, rec, sp, c, D[0], 0.0)
    f.paint_scalar(centre, radius, 7.0, channel=1)                       # on the uploaded records
    m = inside(rec["pos"], centre, radius) & (rec["isGhost"] == 0)
    assert not m[0] and m[1]
    want = c.copy()
    want[m, 1] = F(7.0)
    same_bits(f.scalars(), want, "SET on the uploaded records")
    f.DispatchCompute()                                                  # on the engine's own arrays, at the moved positions
    cur, now = f.scalars(), f.download()
    big = fluid_block(now)[0]
    f.paint_scalar(big, 1.25, 0.5, channel=0, mode=pkg.SPH_SCALAR_ADD)
    m = inside(now["pos"], big, F(1.25)) & (now["isGhost"] == 0)
    assert 20 < m.sum() < (now["isGhost"] == 0).sum()
    want = cur.copy()
    want[m, 0] = (cur[m, 0] + F(0.5)).astype(F)
    same_bits(f.scalars(), want, "ADD on the engine's own arrays")
    assert_records_equal(f.download(), now, "paint does not touch the records")
    for bad in (dict(radius=0.0), dict(radius=np.nan), dict(radius=np.inf), dict(channel=2), dict(channel=-1), dict(mode=2)):
        kw = dict(center=big, radius=1.0, value=1.0, channel=0, mode=pkg.SPH_SCALAR_SET)
        kw.update(bad)
        with pytest.raises(pkg.SphError, match="error -1"):
            f.paint_scalar(**kw)
    same_bits(f.scalars(), want, "a refused paint changes nothing")
    f.close()


def test_moments_match_the_fixed_order_sums(pkg):
    rec, sp, c, D, lam, _, _ = _reference(pkg, "scene4096", 4)
    rec = rec.copy()
    rec["isGhost"][50:70] = 1
    rec["density"][80:90] = 0.0
    c = c.copy()
    c[5, 2] = c[300, 2] = c[:, 2].max() + F(1)                           # a tie: the lower id is reported
    c[7, 3] = np.nan                                                     # a non-finite value is left out of its channel
    f = _scalar_engine(pkg, rec, sp, c, D, lam)
    got = f.scalar_moments()
    now = f.download()
    assert_records_equal(now, rec, "moments do not touch the records")
    same_bits(f.scalars(), c, "moments do not touch the values")
    f.close()
    cells = stats_ref.host_cells(now, pkg.compute_grid_extents(sp))
    want = R.moments(c, R.targets(now), cells)
    assert len(got) == 4
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.count == w["count"], k
        assert np.float64(g.sum).tobytes() == np.float64(w["sum"]).tobytes(), (k, g.sum, w["sum"])
        assert np.float64(g.sum_squares).tobytes() == np.float64(w["sum_squares"]).tobytes(), (k, g.sum_squares, w["sum_squares"])
        assert (F(g.min[0]).tobytes(), g.min[1]) == (F(w["min"][0]).tobytes(), w["min"][1]), k
        assert (F(g.max[0]).tobytes(), g.max[1]) == (F(w["max"][0]).tobytes(), w["max"][1]), k
    assert got[2].max[1] == 5 and got[3].count == got[0].count - 1 and got[0].count == int(R.targets(now).sum())
    var0 = got[0].variance
    assert var0 > 0 and got[0].mixing_index(var0) == 0.0


def test_sampling_matches_the_restatement_and_feeds_the_surface(pkg, oracle):
    torch = pytest.importorskip("torch")
    rec, sp, c, D, lam, _, _ = _reference(pkg, "scene4096", 4)
    f = _scalar_engine(pkg, rec, sp, c, D, lam)
    f.DispatchCompute()
    now, cur = f.download(), f.scalars()
    b = oracle.build_grid(now, to_oracle_params(oracle, sp))
    grid = (b["grid"], b["cell_start"], b["order"])
    g = pkg.compute_grid_extents(sp)
    lo = np.array(list(g.gridMin), F)
    ext = F(g.cellSize) * np.array(list(g.dims), F)
    rng = np.random.default_rng(4)
    pts = np.concatenate([now["pos"][::37, :3], (lo + ext * rng.random((200, 3))).astype(F), (lo - F(1) + (ext + F(2)) * rng.random((40, 3))).astype(F),
                          np.array([[np.nan, 0, 0], [1e20, 1e20, 1e20]], F)]).astype(F)
    for channel in (0, 3):
        got = f.sample_scalar(pts, channel)
        same_bits(got, R.shepard32(now, cur, channel, pts, sp.param_h, *grid), f"point samples of channel {channel}")
        assert (got != 0).sum() > 150 and got[-2] == 0 and got[-1] == 0
    origin, spacing, dims = lo + F(0.11), (F(0.19), F(0.23), F(0.17)), (13, 9, 11)
    lat = f.scalar_lattice(origin, spacing, dims, channel=1)
    assert lat.shape == (11, 9, 13)
    iz, iy, ix = np.meshgrid(np.arange(11), np.arange(9), np.arange(13), indexing="ij")
    lp = np.stack([(origin[0] + (ix.astype(F) * spacing[0]).astype(F)).astype(F), (origin[1] + (iy.astype(F) * spacing[1]).astype(F)).astype(F),
                   (origin[2] + (iz.astype(F) * spacing[2]).astype(F)).astype(F)], axis=-1).reshape(-1, 3)
    same_bits(lat.reshape(-1), R.shepard32(now, cur, 1, lp, sp.param_h, *grid), "lattice samples of channel 1")
    assert_records_equal(f.download(), now, "sampling does not touch the records")
    same_bits(f.scalars(), cur, "sampling does not touch the values")
    # a concentration iso-surface: a painted blob of 1 in a field of 0, meshed at 0.5 from the scalar lattice
    f.set_scalars(np.zeros(len(rec), F), diffusivity=D[0])
    fluid = now["pos"][now["isGhost"] == 0][:, :3]
    blob = fluid.mean(axis=0).astype(F)
    f.paint_scalar(blob, 0.9, 1.0)
    o, s, d = f.default_surface_lattice()
    vol = f.scalar_lattice(o, s, d, channel=0, device=True)
    v, t = f.surface_from_volume(vol, o, s, iso=0.5)
    f.close()
    assert len(v) > 50 and len(t) > 100
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                           # closed: every edge belongs to exactly two triangles


def test_values_none_seeds_the_dye(pkg):
    f = pkg.SPHFluidGPU(6000, params=pkg.default_params(param_dyePattern=1), seed=3)
    f.set_scalars(None, diffusivity=1.0, channels=3)
    rec, c = f.download(), f.scalars()
    assert c.shape == (len(rec), 3) and len(np.unique(rec["padB"])) > 1
    same_bits(c[:, 0], rec["padB"], "channel 0 is padB")
    assert not c[:, 1:].any()
    f.DispatchCompute()
    f.DispatchCompute()
    after = f.download()
    same_bits(after["padB"], rec["padB"], "padB of the records is not rewritten")
    assert (f.scalars()[:, 0] != c[:, 0]).any()
    f.close()


def test_lifetime_and_refusals(pkg):
    rec, sp, c, D, lam, want, _ = _reference(pkg, "scene4096", 1)
    f = _scalar_engine(pkg, rec, sp, c, D, lam)
    dev = f.scalars_device()
    assert dev != 0
    for call in (lambda: f.set_scalars(c[:-1], diffusivity=1.0), lambda: f.set_scalars(np.zeros((len(rec), 5), F), diffusivity=1.0),
                 lambda: f.set_scalars(c, diffusivity=-1.0), lambda: f.set_scalars(c, diffusivity=1.0, decay=np.nan),
                 lambda: f.set_scalars(None, diffusivity=1.0, channels=5), lambda: f.set_scalar_coefficients(diffusivity=np.inf),
                 lambda: f.sample_scalar(np.zeros((1, 3), F), channel=1)):
        with pytest.raises(pkg.SphError, match="error -1"):
            call()
    assert f.num_scalar_channels() == 1 and f.scalars_device() == dev
    f.DispatchCompute()
    same_bits(f.scalars(), want[0], "refused calls changed nothing")
    # SPH_OPT_GRID_BUILD 1 while scalars exist: the next dispatch fails and changes nothing
    before, before_rec = f.scalars(), f.download()
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="error -3"):
        f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="error -3"):
        f.set_scalars(c, diffusivity=1.0)
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    same_bits(f.scalars(), before, "a refused dispatch changes no value")
    assert_records_equal(f.download(), before_rec, "a refused dispatch changes no record")
    assert f.scalar_info()[0] == 1
    # upload and impulses do not touch the values; reset drops the set
    f.upload(before_rec)
    f.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
    same_bits(f.scalars(), before, "upload and impulses")
    f.param_pause = 1
    f.DispatchCompute()
    same_bits(f.scalars(), before, "param_pause")
    assert f.scalar_info()[0] == 1
    f.param_pause = 0
    f.ResetSimulation()
    assert f.num_scalar_channels() == 0 and f.scalars_device() == 0
    with pytest.raises(pkg.SphError, match="error -3"):
        f.paint_scalar((0.0, 0.0, 0.0), 1.0, 1.0)
    f.close()
    # a z-slab engine refuses, before anything is allocated
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    L = pkg.load_library()
    co = np.array([1.0, 0.0], F)
    assert L.sph_scalars_set(slab._h, c.ctypes.data, len(rec), 1, co.ctypes.data_as(C.POINTER(C.c_float))) == -3 and b"slab" in L.sph_last_error()
    assert L.sph_scalars_channels(slab._h) == 0
    slab.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_dye_mixing_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "dye_mixing", tmp_path), ["3", "8000", "4.0"], timeout=120)
    assert res.returncode == 0 and "dye_mixing OK" in res.stdout
    idx = [float(x) for x in re.findall(r"mixing_index=(\S+)", res.stdout)]
    assert len(idx) == 3 and idx[0] > 0 and idx == sorted(idx), idx
