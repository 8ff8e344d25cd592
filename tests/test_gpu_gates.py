"""Flow gates on the GPU (include/sph_abi.h "flow gates").

The engine holds the entry and the exit state of a substep at one slot; a test can only download the state between substeps.  So the
books are checked one step ahead: the records are downloaded around every single dispatch and fed to the host twin
sph_gates_step_host (which tests/test_gates_cpu.py pins to the numpy restatement).  Counts must match exactly; the fp64 sums lie within
coupling_ref.books_bound of the restatement's correctly rounded sums (the terms are exactly defined, only their order is free).
sph_dispatch_n and graph replays, between whose substeps nothing can be downloaded, must leave the bits of the same number of single
dispatches: the kernels and their fixed launch grids are the same."""
import numpy as np
import pytest

from conftest import assert_records_equal, small_scene
import gates_ref as GR
from gates_ref import check_books, mixed_gates
from support import build_example, engine, fluid_block, linked_list_grid, random_scene, run_example, same_bits, slab_engine, undisturbed_run

pytestmark = pytest.mark.gpu

F = np.float32
SCENE = 138          # 5544 particles (a partial wave at the end, several blocks), 277 ghosts, 6 per cell, fast particles, a capsule


def _scene(pkg, seed=SCENE):
    rec, sp, _, what = random_scene(pkg, seed)
    c, E = fluid_block(rec)
    return rec, sp, c, E, what


def _gates(pkg, c, E):
    """Eight gates of mixed shapes: some through the crowded middle of the block, two whole planes, one that nothing reaches."""
    return mixed_gates(pkg, c, 0.5 * E)


def _as_dict(rows):
    return {k: rows[k].copy() for k in ("forward", "backward", "vel", "scalar")}


def _same_books(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], f"{what}: {a} vs {b}"


def _step_ahead(pkg, f, gates, steps, checkpoints, what, K=0):
    """`steps` single dispatches with downloads around each: the engine's books against the twin's at the checkpoints."""
    ref_gates = pkg.gate_array(gates).view(GR.GATE_DTYPE)
    before = f.download()
    twin, total = None, None
    for i in range(1, steps + 1):
        f.DispatchCompute()
        after = f.download()
        vals = f.scalars() if K else None
        twin = pkg.gates_step_host(before, after, gates, vals, twin)
        total = GR.add(total, GR.step(before, after, ref_gates, vals))
        before = after
        if i in checkpoints:
            rows, t, n = f.gate_books()
            assert n == i and abs(t - i * float(F(f.param_timeStep))) <= 1e-12 * i, (what, i, t, n)
            assert rows["forward"].tolist() == twin["forward"].tolist() and rows["backward"].tolist() == twin["backward"].tolist(), \
                f"{what} after {i}: {rows['forward']} {rows['backward']} vs the twin's {twin['forward']} {twin['backward']}"
            check_books(_as_dict(rows), total, f"{what} after {i} (engine)")
            check_books(_as_dict(twin), total, f"{what} after {i} (twin)")
            assert (rows["scalar"][:, K:] == 0).all(), what
    return total


@pytest.mark.parametrize("K", [0, 1, 4])
@pytest.mark.parametrize("aos", [0, 1])
@pytest.mark.parametrize("kern", [1, 2, 3])
def test_books_equal_the_twin(pkg, kern, aos, K):
    rec, sp, c, E, what = _scene(pkg)
    f = engine(pkg, rec, sp, kern, aos)
    try:
        if K:
            f.set_scalars(np.random.default_rng(3).uniform(-1.0, 2.0, (len(rec), K)).astype(F), diffusivity=0.0)
        gates = _gates(pkg, c, E)
        f.set_gates(gates)
        same_bits(f.gates().view(np.uint8), pkg.gate_array(gates).view(np.uint8), "gates as set")
        total = _step_ahead(pkg, f, gates, 64, (1, 7, 64), f"kernel {kern} aos {aos} K {K}", K)
        hits = total["forward"] + total["backward"]
        print(what, "crossings per gate", hits.tolist())
        assert hits[6] == 0 and (hits[:6] > 0).all() and hits[4] > 200, hits       # an empty gate, crossed patches, a busy plane
    finally:
        f.close()


def _hist(f):
    first, rows, times = f.gate_history()
    return first, rows.tobytes(), times.tobytes()


@pytest.mark.parametrize("aos", [0, 1])
def test_dispatch_n_and_graph_replay_equal_single_dispatches(pkg, aos):
    """64 single dispatches, one sph_dispatch_n(64) and four calls of 16 of which the last two replay a graph leave the same books and
    the same history ring; a set_gates between replays is seen by the replay, which needs no new capture."""
    rec, sp, c, E, _ = _scene(pkg)
    gates = _gates(pkg, c, E)
    moved = _gates(pkg, c + F(0.1 * E), E)

    def run(graph, calls):
        f = engine(pkg, rec, sp, 3, aos, graph)
        f.set_gates(gates, history=16, stride=5)
        for n in calls:
            f.DispatchN(n) if n > 1 else f.DispatchCompute()
        return f

    single, whole, replay = run(0, [1] * 64), run(0, [64]), run(1, [16] * 4)
    try:
        want = single.gate_books()
        assert want[2] == 64 and int(want[0]["forward"].sum()) > 200
        launches = replay.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)                            # (a call is captured once it repeats, then replayed)
        assert launches >= 2 and whole.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == 0
        for name, f in (("sph_dispatch_n(64)", whole), ("graph replay", replay)):
            _same_books(f.gate_books(), want, name)
            assert _hist(f) == _hist(single), name
        first, rows, times = single.gate_history()
        assert first == 0 and rows.shape == (12, 8) and (np.diff(times) > 0).all()          # 64 // 5 rows of a ring of 16
        assert (rows[-1]["forward"] <= want[0]["forward"]).all()
        # another table with the same count, history and stride between two replays: books and ring are kept, the replay reads the new table
        for f in (single, replay):
            f.set_gates(moved, history=16, stride=5)
        for _ in range(16):
            single.DispatchCompute()
        replay.DispatchN(16)
        assert replay.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches + 1                # the same graph again, not a first sighting
        _same_books(replay.gate_books(), single.gate_books(), "after set_gates between replays")
        assert _hist(replay) == _hist(single)
        assert single.gate_books()[2] == 80 and single.gate_history()[1].shape == (16, 8)
        # ... and the moved table did count differently from the one before
        still = run(0, [64, 16])
        assert still.gate_books()[0].tobytes() != single.gate_books()[0].tobytes()
        assert_records_equal(still.download(), single.download(), "the records do not depend on the gates")
        assert_records_equal(replay.download(), single.download(), "graph replay")
        still.close()
    finally:
        for f in (single, whole, replay):
            f.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("aos", [0, 1])
def test_gates_do_not_disturb_the_run(pkg, aos, graph):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    c, E = fluid_block(rec)
    gates = _gates(pkg, c, E)
    seen = []

    def probe(f):
        if not len(f.gates()):
            f.set_gates(gates, history=8, stride=2)
        seen.append(f.gate_books()[2])

    want = undisturbed_run(pkg, rec, sp, None, aos, graph)
    got = undisturbed_run(pkg, rec, sp, probe, aos, graph)
    assert_records_equal(got[0], want[0], "after the upload")
    assert_records_equal(got[1], want[1], "at the end")
    assert got[2] == want[2] and max(seen) >= 10                                             # as many graph launches; the books did run


def test_records_scalars_pool_and_tracers_are_untouched(pkg):
    """16 substeps with scalars, sources, buoyancy, a diffuse pool and tracers: every downloadable state is byte-identical with gates."""
    rec, sp, c, E, _ = _scene(pkg)
    rng = np.random.default_rng(9)
    values = rng.uniform(-1.0, 2.0, (len(rec), 2)).astype(F)
    points = (c + rng.uniform(-0.3 * E, 0.3 * E, (64, 3))).astype(F)
    out = []
    for with_gates in (False, True):
        f = engine(pkg, rec, sp, 3, 1)
        f.set_scalars(values, diffusivity=0.0)
        f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.3 * E, channel=1, rate=4.0)])
        f.set_scalar_buoyancy([0.4, -0.2], [0.1, 0.0])
        f.set_diffuse(capacity=4096)
        f.set_tracers(points, history=4, stride=2)
        if with_gates:
            f.set_gates(_gates(pkg, c, E), history=4, stride=3)
        for _ in range(4):
            f.DispatchCompute()
        f.DispatchN(12)
        out.append((f.download(), f.scalars(), f.diffuse(), f.tracers(), f.tracer_history()[1], f.scalar_injected()[0]))
        if with_gates:
            assert f.gate_books()[2] == 16
        f.close()
    assert_records_equal(out[1][0], out[0][0], "records")
    for a, b, name in zip(out[0][1:], out[1][1:], ("scalars", "pool", "tracers", "tracer history", "injected sums")):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def test_lifetimes(pkg):
    rec, sp, c, E, _ = _scene(pkg)
    gates = _gates(pkg, c, E)
    f = engine(pkg, rec, sp)
    g = engine(pkg, rec, sp)
    try:
        assert len(f.gates()) == 0 and f.gate_books()[1:] == (0.0, 0) and f.gate_history()[1].shape[0] == 0
        f.clear_gates()                                                                     # (nothing set: nothing to clear)
        # a ring that wraps: H = 4, S = 3, 20 substeps -> rows after 9, 12, 15 and 18 substeps, the first one is row 2
        f.set_gates(gates, history=4, stride=3)
        g.set_gates(gates)
        f.DispatchN(20)
        want = {}
        for i in range(1, 21):
            g.DispatchCompute()
            if i in (9, 12, 15, 18, 20):
                want[i] = g.gate_books()
        first, rows, times = f.gate_history()
        assert first == 2 and rows.shape == (4, 8)
        for k, i in enumerate((9, 12, 15, 18)):
            assert rows[k].tobytes() == want[i][0].tobytes() and times[k] == want[i][1], f"ring row {k}"
        _same_books(f.gate_books(), want[20], "books after 20")
        # the same count, history and stride keep books and ring; reset=True zeroes the books after the read, not the ring
        f.set_gates(gates[::-1], history=4, stride=3)
        _same_books(f.gate_books(reset=True), want[20], "kept by a set call with the same three")
        rows0, t0, n0 = f.gate_books()
        assert (t0, n0) == (0.0, 0) and not rows0["forward"].any() and not rows0["vel"].any()
        assert f.gate_history()[0] == 2
        f.DispatchCompute()
        assert f.gate_books()[2] == 1 and f.gate_history()[0] == 3                          # (21 substeps since the ring was zeroed: row 6)
        # another count, another history or another stride: books and ring restart
        for args in ((gates[:5], 4, 3), (gates[:5], 8, 3), (gates[:5], 8, 2)):
            f.DispatchN(3)
            assert f.gate_books()[2] > 0
            f.set_gates(args[0], history=args[1], stride=args[2])
            rows0, t0, n0 = f.gate_books()
            assert len(rows0) == 5 and (t0, n0) == (0.0, 0) and not rows0["forward"].any() and f.gate_history()[1].shape == (0, 5), args
        # param_pause: nothing happens, nothing is counted
        f.param_pause = 1
        f.DispatchN(3)
        assert f.gate_books()[2] == 0
        f.param_pause = 0
        f.DispatchN(2)
        assert f.gate_books()[2] == 2 and f.gate_history()[1].shape == (1, 5)
        # sph_reset drops the gates
        f.ResetSimulation()
        assert len(f.gates()) == 0 and f.gate_books()[2] == 0 and f.gate_history()[1].shape[0] == 0
        f.DispatchCompute()
        f.set_gates(gates[:2])
        f.DispatchCompute()
        assert f.gate_books()[2] == 1 and len(f.gate_books()[0]) == 2
    finally:
        f.close()
        g.close()


def test_a_wrapped_ring_is_read_in_two_unequal_pieces(pkg):
    """H = 5, S = 3, 20 substeps: six rows taken, the ring holds rows 1 .. 5 and the oldest of them lies in slot 1, so the read-out is
    slots 1 .. 4 and then slot 0.  Rows and times equal, bit for bit, the books of single dispatches after 6, 9, 12, 15 and 18 substeps."""
    rec, sp, c, E, _ = _scene(pkg)
    gates = _gates(pkg, c, E)
    f, g = engine(pkg, rec, sp), engine(pkg, rec, sp)
    try:
        f.set_gates(gates, history=5, stride=3)
        g.set_gates(gates)
        f.DispatchN(20)
        want = []
        for i in range(1, 19):
            g.DispatchCompute()
            if i % 3 == 0 and i >= 6:
                want.append(g.gate_books())
        first, rows, times = f.gate_history()
        assert first == 1 and rows.shape == (5, 8) and int(rows[-1]["forward"].sum()) > 0
        for k, (books, t, n) in enumerate(want):
            assert rows[k].tobytes() == books.tobytes() and times[k] == t, f"ring row {first + k} (after {n} substeps)"
    finally:
        f.close()
        g.close()


def test_a_recycled_particle_is_not_booked(pkg):
    """The fountain recycles behind the gate step: with every particle recycled across a plane in every substep the books equal those
    of the same substep without the fountain, and the jump itself is no crossing of the next substep either."""
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    c, E = fluid_block(rec)
    top = float(rec["pos"][:, 1].max())
    plane = [pkg.gate(pkg.SPH_GATE_RECT, (float(c[0]), top + 0.5 * float(sp.param_h), float(c[2])), (0, 0, 1), (1, 0, 0), unbounded=True),
             pkg.gate(pkg.SPH_GATE_RECT, c, (0, 0, 1), (1, 0, 0), unbounded=True)]
    half_y = float(sp.param_boxHalf[1])

    def make(records, fountain):
        f = engine(pkg, records, sp)
        f.set_gates(plane)
        if fountain:                                                                        # the jet a cell above the block, everything drains, chance 1
            f.fountainMode = 1
            f.fountainOffset = (0.0, top + 1.5 * float(sp.param_h) - float(sp.param_boxCenter[1]), 0.0)
            f.fountainRadius, f.fountainDrainLevel, f.fountainDrainPerSec = 0.5, 4.0 * half_y, 1e9
        return f

    on, off = make(rec, True), make(rec, False)
    try:
        on.DispatchCompute()
        off.DispatchCompute()
        after_on, after_off = on.download(), off.download()
        jumped = (after_on["pos"][:, 1] != after_off["pos"][:, 1])
        assert jumped.sum() > 3000 and (after_on["pos"][jumped, 1] > top + 0.5 * float(sp.param_h)).all()
        _same_books(on.gate_books(), off.gate_books(), "the gate step runs before the fountain")
        naive = pkg.gates_step_host(rec, after_on, plane)                                   # (what booking the jump would have given)
        assert int(naive["forward"][0]) >= int(jumped.sum()) and int(on.gate_books()[0]["forward"][0]) < 100
        # the next substep starts from the recycled positions
        again = make(after_on, False)
        again.DispatchCompute()
        step2 = pkg.gates_step_host(after_on, again.download(), plane)
        again.close()
        on.fountainMode = 0
        before = on.gate_books()[0]
        on.DispatchCompute()
        rows = on.gate_books()[0]
        assert (rows["forward"] - before["forward"]).tolist() == step2["forward"].tolist()
        assert (rows["backward"] - before["backward"]).tolist() == step2["backward"].tolist()
    finally:
        on.close()
        off.close()


def test_refusals(pkg):
    rec, sp, c, E, _ = _scene(pkg)
    gates = _gates(pkg, c, E)
    with slab_engine(pkg, rec, sp) as slab:
        rc = pkg.load_library().sph_gates_set(slab._h, pkg.gate_array(gates).ctypes.data, len(gates), 0, 1)
        assert rc == -3
    f = engine(pkg, rec, sp)
    try:
        with linked_list_grid(pkg, f):
            with pytest.raises(pkg.SphError, match="error -3"):
                f.set_gates(gates)
        f.set_gates(gates, history=4, stride=2)
        f.DispatchCompute()
        held, state = f.gate_books(), f.download()
        with linked_list_grid(pkg, f):                                                      # the option while gates exist: the dispatch fails and changes nothing
            with pytest.raises(pkg.SphError, match="error -3"):
                f.DispatchCompute()
            with pytest.raises(pkg.SphError, match="error -3"):
                f.DispatchN(3)
        _same_books(f.gate_books(), held, "a refused dispatch")
        assert_records_equal(f.download(), state, "a refused dispatch")
        # SPH_ERR_ARG with the previous state kept
        R = pkg.SPH_GATE_RECT
        ok = pkg.gate(R, c, (1, 0, 0), (0, 1, 0))
        bad_shape, bad_flag, nan, zero = (pkg.gate(R, c, (1, 0, 0), (0, 1, 0)) for _ in range(4))
        bad_shape.shape, bad_flag.flags, nan.center[2] = 7, 4, np.nan
        zero.u[0] = 0.0
        skew = pkg.gate(R, c, (1, 0, 0), (0.01, 1, 0))
        for args in (([ok] * 9, 0, 1), ([bad_shape], 0, 1), ([bad_flag], 0, 1), ([nan], 0, 1), ([zero], 0, 1), ([skew], 0, 1), ([ok], 4097, 1), ([ok], 4, 0)):
            with pytest.raises(pkg.SphError, match="error -1"):
                f.set_gates(args[0], history=args[1], stride=args[2])
        assert pkg.load_library().sph_gates_set(f._h, None, 3, 0, 1) == -1                  # a null table with a count > 0
        same_bits(f.gates().view(np.uint8), pkg.gate_array(gates).view(np.uint8), "the previous table stays")
        _same_books(f.gate_books(), held, "refused set calls")
        f.DispatchCompute()
        assert f.gate_books()[2] == 2 and f.gate_history()[1].shape == (1, 8)
    finally:
        f.close()


def test_control_volume_example(pkg, tmp_path):
    exe = build_example(pkg, "control_volume", tmp_path, werror=True)
    res = run_example(exe, [4, 20000], timeout=120)
    assert res.returncode == 0 and "control_volume OK" in res.stdout, res.stdout + res.stderr


def test_scalar_flux_sees_this_substeps_sources_and_kick(pkg):
    """The order against the coupling step: with a source and buoyancy on, the books of a whole plane hold the values AFTER this
    substep's sources and the velocity AFTER the kick -- what the download after the substep shows, which the twin is fed."""
    rec, sp, c, E, _ = _scene(pkg)
    f = engine(pkg, rec, sp)
    try:
        f.set_scalars(np.zeros((len(rec), 1), F), diffusivity=0.0)
        f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_BOX, c, (E, E, E), channel=0, mode=pkg.SPH_SOURCE_RATE, rate=1000.0)])
        f.set_scalar_buoyancy([0.5], [0.0])
        plane = [pkg.gate(pkg.SPH_GATE_RECT, c, (0, 0, 1), (1, 0, 0), unbounded=True)]
        f.set_gates(plane)
        total = _step_ahead(pkg, f, plane, 6, (1, 6), "sources and buoyancy on", K=1)
        hits = int(total["forward"][0] + total["backward"][0])
        # every crosser carried dt * rate per substep it has lived through: the books can only match with the sources applied first
        assert hits > 50 and total["abs_scalar"][0, 0] >= hits * float(F(sp.param_timeStep) * F(1000.0)) * 0.999
    finally:
        f.close()
