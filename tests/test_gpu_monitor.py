"""Field monitors on the GPU (include/sph_abi.h "field monitors").

A monitor sample is, bit for bit, sample() called just before the dispatch: the tests call it there, feed the acting substeps' samples to
the host twin sph_monitor_accumulate_host (which tests/test_monitor_cpu.py pins to the numpy restatement) and compare bytes.  Every
comparison is byte equality.  sph_dispatch_n and graph replays, between whose substeps nothing can be sampled, must leave the bytes of
the same number of single dispatches."""
import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import monitor_ref as MR
from gates_ref import mixed_gates
from support import build_example, engine, fluid_block, linked_list_grid, random_scene, run_example, same_bits, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu

F = np.float32
SCENE = 138          # 5544 particles (a partial wave at the end, several blocks), 277 ghosts, 6 per cell, fast particles, a capsule
STAGE_RECORDS = 1024  # kStageF4 = 2048 float4 of LDS staging per block, two float4 per record when the velocity is sampled


def _scene(pkg, seed=SCENE):
    rec, sp, _, what = random_scene(pkg, seed)
    c, E = fluid_block(rec)
    return rec, sp, c, E, what


def _probes(pkg, rec, sp, c, E, m=203, seed=4):
    """m points (a partial last wave): most of them within a fifth of h of the fluid block's faces, where the Shepard fraction hovers
    around one half, the rest in and around the block; a NaN point, a point outside the grid on each of its six sides, points exactly
    on cell faces, and one point given twice."""
    rng = np.random.default_rng(seed)
    g = pkg.compute_grid_extents(sp)
    gmin, cell, dims = np.array(list(g.gridMin), F), F(g.cellSize), np.array(list(g.dims))
    fluid = rec["pos"][rec["isGhost"] == 0][:, :3]
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    pts = (c + rng.uniform(-0.7 * E, 0.7 * E, (m, 3))).astype(F)
    near = np.arange(m) < (2 * m) // 3                                           # on a face of the block's bounding box, jittered
    inside = (lo + rng.random((m, 3)) * (hi - lo)).astype(F)
    axis, side = rng.integers(0, 3, m), rng.integers(0, 2, m)
    inside[np.arange(m), axis] = np.where(side == 1, hi[axis], lo[axis]) + rng.uniform(-0.2, 0.2, m).astype(F) * F(sp.param_h)
    pts[near] = inside[near]
    k = m - 12
    pts[k] = (np.nan, c[1], c[2])
    for a in range(3):
        pts[k + 1 + 2 * a] = c
        pts[k + 1 + 2 * a, a] = gmin[a] - F(2.5) * cell
        pts[k + 2 + 2 * a] = c
        pts[k + 2 + 2 * a, a] = gmin[a] + F(dims[a] + 2.5) * cell
    for j in range(4):                                                           # exactly on cell faces (all three coordinates)
        pts[k + 7 + j] = gmin + (rng.integers(1, np.maximum(dims - 1, 2), 3)).astype(F) * cell
    pts[k + 11] = pts[0]
    return pts


def _times(f, n):
    """The fp64 time of the entry state of substeps 0 .. n-1: the running sum of (double)dt."""
    out, t = [], 0.0
    for _ in range(n):
        out.append(t)
        t = t + float(F(f.param_timeStep))
    return out


def _step_ahead(pkg, f, sampler, slot, steps, every, checkpoints, what, history=0, stride=1, ring_points=0):
    """`steps` single dispatches with sampler() before each: rows, info and ring of the slot against the twin at the checkpoints."""
    twin, taken, acting = None, [], 0
    times = _times(f, steps)
    for i in range(1, steps + 1):
        s = sampler()
        if (i - 1) % every == 0:
            twin = pkg.monitor_accumulate_host(twin, s, f.monitor_info(slot)["wetFraction"])
            if history and acting % stride == 0:
                taken.append((s.reshape(-1)[:ring_points].copy(), times[i - 1]))
            acting += 1
        f.DispatchCompute()
        if i in checkpoints:
            rows, info = f.monitor_rows(slot), f.monitor_info(slot)
            assert (info["substeps"], info["acting"]) == (i, acting) and info["time"] == times[i - 1] + float(F(f.param_timeStep)), (what, i, info)
            same_bits(rows.view(np.uint8), twin.reshape(rows.shape).view(np.uint8), f"{what}: rows after {i}")
            if history:
                first, samples, tm = f.monitor_history(slot)
                held = taken[-history:]
                assert first == len(taken) - len(held) == info["firstRow"] and len(samples) == len(held) == info["ringRows"], (what, i, first, len(samples))
                for k, (want, t) in enumerate(held):
                    same_bits(samples[k].view(np.uint8), want.view(np.uint8), f"{what}: ring row {first + k} after {i}")
                    assert tm[k] == t, (what, i, k)
    return twin


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("aos", [0, 1])
@pytest.mark.parametrize("kern", [1, 2, 3])
def test_rows_equal_the_twin(pkg, kern, aos, every):
    rec, sp, c, E, what = _scene(pkg)
    pts = _probes(pkg, rec, sp, c, E)
    f = engine(pkg, rec, sp, kern, aos)
    try:
        f.set_monitor(pts, every=every, history=3, stride=2, ring_points=70)
        info = f.monitor_info()
        assert (info["kind"], info["points"], info["dims"], info["every"], info["history"], info["stride"], info["ringPoints"]) == \
            (pkg.SPH_MONITOR_POINTS, 203, (203, 1, 1), every, 3, 2, 70)
        twin = _step_ahead(pkg, f, lambda: f.sample(pts), 0, 24, every, (1, 7, 24), f"kernel {kern} aos {aos} every {every}", 3, 2, 70)
        acting = (24 + every - 1) // every
        mixed = (twin["wet"] > 0) & (twin["wet"] < twin["samples"])
        print(what, f"every {every}: {int(mixed.sum())} of 203 points with 0 < wet < samples; wet anywhere {int((twin['wet'] > 0).sum())}")
        assert (twin["samples"] == acting).all() and twin["wet"][191] == 0         # (the NaN point: an all-zero record every time, dry)
        same_bits(twin[202:203].view(np.uint8), twin[0:1].view(np.uint8), "the point given twice")
        assert mixed.sum() * 3 >= 203, "both branches must accumulate at a third of the points"
    finally:
        f.close()


def _brick_records(rec, g, origin, spacing, dims):
    """Per 8 x 8 x 4 brick of the lattice, the records in the brick's cell range +-1 (what k_monitor_lattice would stage), from the
    cell formula floor((x - gridMin) / cellSize) clamped to the grid, in float32."""
    gmin, cell, gd = np.array(list(g.gridMin), F), F(g.cellSize), np.array(list(g.dims))

    def cells(x, a):
        return np.clip(np.floor((np.asarray(x, F) - gmin[a]) / cell), 0, gd[a] - 1).astype(int)
    pc = np.stack([cells(rec["pos"][:, a], a) for a in range(3)], axis=1)
    counts = np.zeros(tuple(gd[::-1]), int)
    np.add.at(counts, (pc[:, 2], pc[:, 1], pc[:, 0]), 1)
    out, rows = [], []
    for bz in range(0, dims[2], 4):
        for by in range(0, dims[1], 8):
            for bx in range(0, dims[0], 8):
                rng_ = []
                for a, (b0, n) in enumerate(((bx, 8), (by, 8), (bz, 4))):
                    i0, i1 = b0, min(b0 + n, dims[a]) - 1
                    x0, x1 = F(origin[a]) + F(i0) * F(spacing[a]), F(origin[a]) + F(i1) * F(spacing[a])
                    rng_.append((max(int(cells(x0, a)) - 1, 0), min(int(cells(x1, a)) + 1, gd[a] - 1)))
                (x0, x1), (y0, y1), (z0, z1) = rng_
                out.append(int(counts[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1].sum()))
                rows.append((y1 - y0 + 1) * (z1 - z0 + 1))
    return np.array(out), np.array(rows)


@pytest.mark.parametrize("fine", [True, False])
def test_lattice_monitor_equals_the_twin_and_an_explicit_monitor(pkg, fine):
    """Dims (19, 13, 9): partial bricks on every axis; the origin 1.5 cells outside the grid on the low side in x and z, and 1.5 cells
    below the fluid in y (the grid reaches six empty cells below the fluid: a lattice begun outside it there would see none).  A block
    stages kStageF4 = 2048 float4 = 1024 records (two float4 each with the velocity) in at most 64 rows.  The lattice covers the low
    corner of the fluid, where the block's 6 particles per cell begin one cell inside the grid:
      cell / 2: a brick spans 3.5 (x, y) and 1.5 (z) cells, +-1: at most 7 x 7 x 5 cells of which the corner leaves most empty; the
                fullest brick has 459 records in 21 rows: every brick stages;
      cell:     a brick spans 7 (x, y) and 3 (z) cells, +-1: up to 10 x 10 x 6 cells; the fullest bricks have 1198, 1327 and 1366
                records in 60 rows and walk global memory, the emptiest (27) stages.
    The counts are recomputed below on the scene itself, with a quarter of margin either way for the substeps the particles move."""
    rec, sp, c, E, what = _scene(pkg)
    g = pkg.compute_grid_extents(sp)
    cell = F(g.cellSize)
    dims = (19, 13, 9)
    spacing = np.full(3, cell / F(2) if fine else cell, F)
    origin = np.array(list(g.gridMin), F) - F(1.5) * cell
    origin[1] = rec["pos"][rec["isGhost"] == 0][:, 1].min() - F(1.5) * cell
    per_brick, rows = _brick_records(rec, g, origin, spacing, dims)
    print(what, "fine" if fine else "coarse", "records per brick", per_brick.tolist(), "rows", rows.tolist())
    assert (rows <= 64).all()
    if fine:
        assert per_brick.max() <= 0.75 * STAGE_RECORDS and per_brick.max() > 0
    else:
        assert per_brick.max() >= 1.25 * STAGE_RECORDS and per_brick.min() <= 0.75 * STAGE_RECORDS
    idx = [np.arange(n, dtype=F) for n in dims]
    pts = np.zeros(dims[::-1] + (4,), F)                                         # the lattice's points: origin + (float)i * spacing
    pts[..., 0] = (origin[0] + idx[0] * spacing[0])[None, None, :]
    pts[..., 1] = (origin[1] + idx[1] * spacing[1])[None, :, None]
    pts[..., 2] = (origin[2] + idx[2] * spacing[2])[:, None, None]
    f = engine(pkg, rec, sp)
    try:
        f.set_monitor(lattice=(origin, spacing, dims), slot=2, every=2, history=2, stride=1, ring_points=100)
        f.set_monitor(pts.reshape(-1, 4), slot=1, every=2, history=2, stride=1, ring_points=100)
        info = f.monitor_info(2)
        assert (info["kind"], info["points"], info["dims"]) == (pkg.SPH_MONITOR_LATTICE, 19 * 13 * 9, dims)
        twin = _step_ahead(pkg, f, lambda: f.sample_lattice(origin, spacing, dims, field=pkg.SPH_FIELD_ALL), 2, 9, 2, (1, 4, 9),
                           "lattice " + ("fine" if fine else "coarse"), 2, 1, 100)
        lat, exp = f.monitor_rows(2), f.monitor_rows(1)
        assert lat.shape == (9, 13, 19) and exp.shape == (19 * 13 * 9,)
        same_bits(lat.reshape(-1).view(np.uint8), exp.view(np.uint8), "lattice monitor vs explicit monitor")
        assert [f.monitor_info(s)[k] for s in (1, 2) for k in ("substeps", "acting", "time")] == [9, 5, f.monitor_info(1)["time"]] * 2
        h1, h2 = f.monitor_history(1), f.monitor_history(2)
        assert h1[0] == h2[0] == 3 and h1[1].tobytes() == h2[1].tobytes() and h1[2].tobytes() == h2[2].tobytes()
        assert (twin["wet"] > 0).sum() > 50 and (twin["wet"] == 0).sum() > 50      # the lattice sees fluid and air
    finally:
        f.close()


def _state(f, slot=0):
    first, samples, times = f.monitor_history(slot)
    return f.monitor_rows(slot).tobytes(), sorted(f.monitor_info(slot).items()), first, samples.tobytes(), times.tobytes()


@pytest.mark.parametrize("aos", [0, 1])
def test_dispatch_n_and_graph_replay_equal_single_dispatches(pkg, aos):
    """48 single dispatches, one sph_dispatch_n(48) and four calls of 12 of which the later ones replay a graph leave the same rows,
    info and ring (every 5, history 4, stride 2: ten acting substeps, five ring rows, the ring wraps); reset_monitor between two
    replays needs no new capture and is seen by the replay."""
    rec, sp, c, E, _ = _scene(pkg)
    pts = _probes(pkg, rec, sp, c, E)
    g = pkg.compute_grid_extents(sp)
    lattice = (np.array(list(g.gridMin), F), np.full(3, F(g.cellSize) * F(0.5), F), (9, 10, 5))

    def run(graph, calls):
        f = engine(pkg, rec, sp, 3, aos, graph)
        f.set_monitor(pts, every=5, history=4, stride=2)
        f.set_monitor(lattice=lattice, slot=3, every=5, history=4, stride=2, ring_points=9)
        for n in calls:
            f.DispatchN(n) if n > 1 else f.DispatchCompute()
        return f

    single, whole, replay = run(0, [1] * 48), run(0, [48]), run(1, [12] * 4)
    try:
        info = single.monitor_info()
        assert (info["substeps"], info["acting"], info["ringRows"], info["firstRow"], info["ringPoints"]) == (48, 10, 4, 1, 64)
        assert (np.diff(single.monitor_history()[2]) > 0).all() and single.monitor_rows()["wet"].sum() > 200
        launches = replay.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)                    # (a call is captured once it repeats, then replayed)
        assert launches >= 2 and whole.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == 0
        for name, f in (("sph_dispatch_n(48)", whole), ("graph replay", replay)):
            for slot in (0, 3):
                assert _state(f, slot) == _state(single, slot), f"{name} slot {slot}"
        # a reset between two replays: rows, counters and ring restart on the stream, the same graph runs again
        for f in (single, replay):
            f.reset_monitor()
        zero = single.monitor_info()
        assert (zero["substeps"], zero["acting"], zero["time"], zero["ringRows"]) == (0, 0, 0.0, 0) and not single.monitor_rows().tobytes().strip(b"\0")
        for _ in range(12):
            single.DispatchCompute()
        replay.DispatchN(12)
        assert replay.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches + 1        # the same graph again, not a first sighting
        for slot in (0, 3):
            assert _state(replay, slot) == _state(single, slot), f"after reset_monitor between replays, slot {slot}"
        assert single.monitor_info()["substeps"] == 12 and single.monitor_info(3)["substeps"] == 60
        # a set call that keeps kind, M and ring layout needs no new capture either, and the replay reads the new points
        moved = pts + F(0.05 * E)
        for f in (single, replay):
            f.set_monitor(moved, every=5, history=4, stride=2)
        for _ in range(12):
            single.DispatchCompute()
        replay.DispatchN(12)
        assert replay.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches + 2
        assert _state(replay) == _state(single)
        assert_records_equal(replay.download(), single.download(), "graph replay")
    finally:
        for f in (single, whole, replay):
            f.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("aos", [0, 1])
def test_monitors_do_not_disturb_the_run(pkg, aos, graph):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    c, E = fluid_block(rec)
    pts = _probes(pkg, rec, sp, c, E)
    seen = []

    def probe(f):
        if f.monitor_info()["kind"] == pkg.SPH_MONITOR_NONE:
            f.set_monitor(pts, every=2, history=8, stride=2)
            f.set_monitor(lattice=(c - F(0.4 * E), F(0.1 * E), (9, 9, 9)), slot=1)
        seen.append(f.monitor_info()["substeps"])

    want = undisturbed_run(pkg, rec, sp, None, aos, graph)
    got = undisturbed_run(pkg, rec, sp, probe, aos, graph)
    assert_records_equal(got[0], want[0], "after the upload")
    assert_records_equal(got[1], want[1], "at the end")
    assert got[2] == want[2] and max(seen) >= 10                                    # as many graph launches; the monitors did run


def test_every_other_state_is_untouched(pkg):
    """16 substeps with scalars, sources, buoyancy, a diffuse pool, tracers and gates: every downloadable state is byte-identical
    with monitors on."""
    rec, sp, c, E, _ = _scene(pkg)
    rng = np.random.default_rng(9)
    values = rng.uniform(-1.0, 2.0, (len(rec), 2)).astype(F)
    points = (c + rng.uniform(-0.3 * E, 0.3 * E, (64, 3))).astype(F)
    out = []
    for with_monitors in (False, True):
        f = engine(pkg, rec, sp, 3, 1)
        f.set_scalars(values, diffusivity=0.0)
        f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.3 * E, channel=1, rate=4.0)])
        f.set_scalar_buoyancy([0.4, -0.2], [0.1, 0.0])
        f.set_diffuse(capacity=4096)
        f.set_tracers(points, history=4, stride=2)
        f.set_gates(mixed_gates(pkg, c, 0.5 * E), history=4, stride=3)
        if with_monitors:
            f.set_monitor(_probes(pkg, rec, sp, c, E), history=4, stride=3)
            f.set_monitor(lattice=(c - F(0.4 * E), F(0.1 * E), (9, 9, 9)), slot=3, every=3)
        for _ in range(4):
            f.DispatchCompute()
        f.DispatchN(12)
        out.append((f.download(), f.scalars(), f.diffuse(), f.tracers(), f.tracer_history()[1], f.gate_books()[0], f.gate_history()[1], f.scalar_injected()[0]))
        if with_monitors:
            assert f.monitor_info()["acting"] == 16 and f.monitor_info(3)["acting"] == 6
        f.close()
    assert_records_equal(out[1][0], out[0][0], "records")
    for a, b, name in zip(out[0][1:], out[1][1:], ("scalars", "pool", "tracers", "tracer history", "gate books", "gate history", "injected sums")):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_lifetimes(pkg):
    rec, sp, c, E, _ = _scene(pkg)
    pts = _probes(pkg, rec, sp, c, E)
    f = engine(pkg, rec, sp)
    try:
        empty = f.monitor_info(2)
        assert empty["kind"] == pkg.SPH_MONITOR_NONE and not any(v for k, v in empty.items() if k not in ("dims", "origin", "spacing")) and empty["dims"] == (0, 0, 0)
        assert f.monitor_rows(2).shape == (0,) and f.monitor_history(2)[1].shape[0] == 0 and f.monitor_rows(2, device=True) == 0
        f.clear_monitor()                                                           # (nothing set: nothing to clear)
        f.clear_monitor(1)
        f.set_monitor(pts, slot=0, every=2)
        f.set_monitor(pts[:50], slot=2, history=3)
        f.DispatchN(5)
        assert (f.monitor_info(0)["acting"], f.monitor_info(2)["acting"], f.monitor_info(2)["ringRows"]) == (3, 5, 3)
        assert f.monitor_rows(0, device=True) != 0
        # param_pause: nothing happens, nothing is counted
        held0, held2 = _state(f, 0), _state(f, 2)
        f.param_pause = 1
        f.DispatchN(3)
        f.DispatchCompute()
        assert _state(f, 0) == held0 and _state(f, 2) == held2
        f.param_pause = 0
        # a set on one slot restarts that slot and leaves the others alone
        f.set_monitor(pts[:10], slot=1)
        f.set_monitor(pts[:50], slot=2, history=3)
        assert _state(f, 0) == held0 and f.monitor_info(2)["substeps"] == 0 and not f.monitor_rows(2).tobytes().strip(b"\0")
        f.DispatchCompute()
        assert [f.monitor_info(s)["substeps"] for s in range(4)] == [6, 1, 1, 0]
        # the first substep after a set samples the state at set time
        s = f.sample(pts[:10])
        f.set_monitor(pts[:10], slot=1, history=1)
        f.DispatchCompute()
        same_bits(f.monitor_history(1)[1][0].view(np.uint8), s.view(np.uint8), "the state at set time")
        # clear one slot, then all
        f.clear_monitor(0)
        assert [f.monitor_info(s)["kind"] for s in range(4)] == [0, 1, 1, 0]
        f.DispatchCompute()
        assert f.monitor_info(2)["substeps"] == 3
        f.clear_monitor()
        assert [f.monitor_info(s)["kind"] for s in range(4)] == [0, 0, 0, 0]
        f.DispatchCompute()
        # sph_reset drops every slot
        f.set_monitor(pts, slot=0)
        f.set_monitor(lattice=(c, F(0.1 * E), (3, 2, 1)), slot=3)
        assert f.monitor_rows(3).shape == (1, 2, 3)
        f.ResetSimulation()
        assert [f.monitor_info(s)["kind"] for s in range(4)] == [0, 0, 0, 0]
        f.DispatchCompute()
        f.set_monitor(pts[:5])
        f.DispatchCompute()
        assert f.monitor_info()["substeps"] == 1 and (f.monitor_rows()["samples"] == 1).all()
    finally:
        f.close()


def test_refusals(pkg):
    rec, sp, c, E, _ = _scene(pkg)
    pts = _probes(pkg, rec, sp, c, E)
    p4 = np.zeros((len(pts), 4), F)
    p4[:, :3] = pts
    L = pkg.load_library()
    o3, s3 = np.zeros(3, F), np.ones(3, F)
    d3 = np.array([3, 3, 3], np.int32)

    def lattice(h, slot, o=o3, s=s3, d=d3, cfg=None):
        return L.sph_monitor_set_lattice(h, slot, o.ctypes.data_as(L.sph_monitor_set_lattice.argtypes[2]), s.ctypes.data_as(L.sph_monitor_set_lattice.argtypes[3]),
                                         d.ctypes.data_as(L.sph_monitor_set_lattice.argtypes[4]), cfg)
    with slab_engine(pkg, rec, sp) as slab:
        assert L.sph_monitor_set(slab._h, 0, p4.ctypes.data, len(p4), None) == -3
        assert lattice(slab._h, 0) == -3
    f = engine(pkg, rec, sp)
    try:
        with linked_list_grid(pkg, f):
            with pytest.raises(pkg.SphError, match="error -3"):
                f.set_monitor(pts)
            with pytest.raises(pkg.SphError, match="error -3"):
                f.set_monitor(lattice=(o3, s3, d3))
        assert f.monitor_info()["kind"] == pkg.SPH_MONITOR_NONE
        f.set_monitor(pts, every=2, history=4, stride=2)
        f.set_monitor(lattice=(c, F(0.1 * E), (4, 3, 2)), slot=1)
        f.DispatchCompute()
        held, state = (_state(f, 0), _state(f, 1)), f.download()
        with linked_list_grid(pkg, f):                                              # the option while a monitor exists: the dispatch fails and changes nothing
            with pytest.raises(pkg.SphError, match="error -3"):
                f.DispatchCompute()
            with pytest.raises(pkg.SphError, match="error -3"):
                f.DispatchN(3)
        assert (_state(f, 0), _state(f, 1)) == held
        assert_records_equal(f.download(), state, "a refused dispatch")
        # SPH_ERR_ARG with the previous state kept
        cfg = pkg.monitor_config
        for kw in (dict(slot=-1), dict(slot=4), dict(every=0), dict(stride=0), dict(history=4097), dict(history=2, ring_points=204),
                   dict(wet_fraction=np.nan), dict(wet_fraction=np.inf)):
            with pytest.raises(pkg.SphError, match="error -1"):
                f.set_monitor(pts, **kw)
        for slot in (0, 1):
            assert L.sph_monitor_set(f._h, slot, None, 3, None) == -1                # null data with m > 0
            assert L.sph_monitor_set_device(f._h, slot, None, 3, None) == -1
            assert L.sph_monitor_set(f._h, slot, p4.ctypes.data, 4194305, None) == -1   # m above the cap (refused before the data is read)
            assert lattice(f._h, slot, d=np.array([4194305, 1, 1], np.int32)) == -1   # the lattice's point count above the cap
            assert lattice(f._h, slot, d=np.array([2048, 2048, 2], np.int32)) == -1
            assert lattice(f._h, slot, d=np.array([3, 0, 3], np.int32)) == -1         # a dim < 1
            for s in (np.array([1, 0, 1], F), np.array([1, 1, -1], F), np.array([np.nan, 1, 1], F), np.array([1, np.inf, 1], F)):
                assert lattice(f._h, slot, s=s) == -1                                 # a spacing not finite and > 0
            for o in (np.array([np.nan, 0, 0], F), np.array([0, -np.inf, 0], F)):
                assert lattice(f._h, slot, o=o) == -1                                 # an origin not finite
            for kw in (dict(every=0), dict(stride=0), dict(history=4097), dict(history=2, ringPoints=28), dict(wetFraction=np.nan)):
                assert lattice(f._h, slot, cfg=cfg(**kw)) == -1, kw
            # a ring over the byte cap: 4096 rows of 2049 samples of 32 bytes is 256 MiB + 128 KiB (2048 samples fit exactly)
            assert lattice(f._h, slot, d=np.array([2049, 1, 1], np.int32), cfg=cfg(history=4096, ringPoints=2049)) == -1
        assert lattice(f._h, 4) == -1 and lattice(f._h, -1) == -1
        assert L.sph_monitor_field(f._h, 0, 10, None) == -1 and L.sph_monitor_field(f._h, 0, -1, None) == -1 and L.sph_monitor_field(f._h, 2, 0, None) == -3
        assert L.sph_monitor_reset(f._h, 2) == -3 and L.sph_monitor_reset(f._h, 7) == -1 and L.sph_monitor_clear(f._h, 4) == -1
        # SPH_ERR_CAPACITY from the download calls
        rows = np.zeros(203, pkg.MONITOR_ROW_DTYPE)
        assert L.sph_monitor_download(f._h, 0, rows.ctypes.data, 202) == -4 and L.sph_monitor_download(f._h, 0, rows.ctypes.data, 203) == 0
        f.DispatchN(4)
        buf, tm = np.zeros((2, 64), pkg.SAMPLE_DTYPE), np.zeros(2)
        assert L.sph_monitor_history(f._h, 0, None, None, buf.ctypes.data, tm.ctypes.data, 1) == -4
        assert L.sph_monitor_history(f._h, 0, None, None, buf.ctypes.data, tm.ctypes.data, 2) == 0 and tm[1] > tm[0] == 0.0
        # after all of it the previous monitors are intact and a following dispatch still counts
        assert [f.monitor_info(s)[k] for s in (0, 1) for k in ("kind", "points", "substeps", "acting")] == [1, 203, 5, 3, 2, 24, 5, 5]
        assert f.monitor_info()["every"] == 2 and f.monitor_info()["history"] == 4
        f.DispatchCompute()
        assert f.monitor_info()["substeps"] == 6 and f.monitor_info(1)["acting"] == 6
    finally:
        f.close()


def test_fields_and_the_mean_free_surface(pkg):
    rec, sp, c, E, _ = _scene(pkg)
    pts = _probes(pkg, rec, sp, c, E)
    g = pkg.compute_grid_extents(sp)
    cell = F(g.cellSize)
    origin, spacing, dims = np.array(list(g.gridMin), F) + F(0.5) * cell, np.full(3, F(0.5) * cell, F), tuple(int(2 * d - 2) for d in g.dims)
    f = engine(pkg, rec, sp)
    try:
        f.set_monitor(pts)
        f.set_monitor(lattice=(origin, spacing, dims), slot=1, every=2)
        f.DispatchN(14)
        for slot in (0, 1):
            rows = f.monitor_rows(slot)
            for which in range(pkg.SPH_MONITOR_FIELDS):
                got = f.monitor_field(which, slot)
                assert got.shape == rows.shape and got.dtype == np.float32
                same_bits(got.view(np.uint32), pkg.monitor_field_host(rows, which).view(np.uint32), f"slot {slot} field {which}")
                same_bits(got.view(np.uint32), MR.field(rows, which).reshape(rows.shape).view(np.uint32), f"slot {slot} field {which} (restatement)")
            assert (f.monitor_field(pkg.SPH_MONITOR_TKE, slot) > 0).any() and (f.monitor_field(pkg.SPH_MONITOR_VAR_PRESSURE, slot) > 0).any()
        vol = f.monitor_field(pkg.SPH_MONITOR_MEAN_FRACTION, 1, device=True)
        assert tuple(vol.shape) == dims[::-1]
        verts, tris = f.surface_from_volume(vol, origin, spacing, iso=0.5)
        hi = origin + (np.array(dims, F) - 1) * spacing
        print("mean free surface:", len(verts), "vertices", len(tris), "triangles")
        assert len(verts) > 0 and len(tris) > 0
        assert (verts["pos"] >= origin - 1e-4).all() and (verts["pos"] <= hi + 1e-4).all()
        m = pkg.monitor_means(f.monitor_rows(1))
        assert np.nanmax(np.abs(m["vel"])) > 0 and np.allclose(np.nan_to_num(m["fraction"]), f.monitor_field(pkg.SPH_MONITOR_MEAN_FRACTION, 1), rtol=1e-6, atol=1e-7)
    finally:
        f.close()


def test_mean_flow_example(pkg, tmp_path):
    exe = build_example(pkg, "mean_flow", tmp_path, werror=True)
    res = run_example(exe, [3, 20000], timeout=120)
    assert res.returncode == 0 and "mean_flow OK" in res.stdout, res.stdout + res.stderr
