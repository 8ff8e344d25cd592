"""Spray, foam and bubbles on the GPU: the pool after n substeps against the host loop
    s = sample(pool.pos); P = download(); dispatch(dt); pool = diffuse_step_host(pool, s, P, ...)
run on a second engine that holds no pool, and against the numpy restatement (tests/diffuse_ref.py, whose scene
tests/test_diffuse_cpu.py shows to contain every event).  Everything is compared bit for bit, order included; no tolerance is used."""
import ctypes as C
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, to_oracle_params
import diffuse_ref as D
from support import build_example, engine, run_example

pytestmark = pytest.mark.gpu

F = np.float32
INFO_KEYS = ("substeps", "spawned", "dropped", "diedLife", "diedAge", "leftBox", "nonFinite", "seeded", "alive", "aliveByKind")


def _cfg(pkg, **kw):
    return pkg.diffuse_config(**dict(D.SCENE_CONFIG, **kw))


def _totals(pool):
    return {"seeded": len(pool), "alive": len(pool)}


def _host_step(pkg, h, cfg, pool, totals, dt=-1.0):
    """One turn of the host loop on the engine h (which holds no pool)."""
    s = h.sample(pool["pos"]) if len(pool) else np.zeros(0, pkg.SAMPLE_DTYPE)
    P = h.download()
    h.DispatchCompute(dt)
    return pkg.diffuse_step_host(cfg, h.params, pool, s, P, totals.get("substeps", 0), dt=dt, totals=totals)


def _same_pool(f, pool, totals, what):
    got = f.diffuse()
    assert len(got) == len(pool), f"{what}: {len(got)} records, the host loop has {len(pool)}"
    if got.tobytes() != pool.tobytes():
        for name in got.dtype.names:
            bad = np.nonzero((got[name] != pool[name]) & ~((got[name] != got[name]) & (pool[name] != pool[name])))[0]
            if len(bad):
                raise AssertionError(f"{what}: field {name} differs in {len(bad)} records, first {bad[0]}: {got[name][bad[0]]} vs {pool[name][bad[0]]}")
        raise AssertionError(f"{what}: pools differ")
    info = f.diffuse_info()
    assert {k: info[k] for k in INFO_KEYS} == {k: totals[k] for k in INFO_KEYS}, f"{what}: {info} vs {totals}"
    gone = sum(info[k] for k in ("dropped", "diedLife", "diedAge", "leftBox", "nonFinite"))
    assert info["alive"] == info["seeded"] + info["spawned"] - gone <= info["capacity"], what


def _pair(pkg, rec, sp, cfg, pool, **kw):
    f, h = engine(pkg, rec, sp, **kw), engine(pkg, rec, sp)
    f.set_diffuse(cfg)
    f.seed_diffuse(pool)
    return f, h


@pytest.mark.parametrize("capacity", [None, 64])
def test_pool_equals_the_host_loop_and_the_reference(pkg, oracle, capacity):
    rec, sp, op, pool = D.scene(pkg, oracle)
    cfg = _cfg(pkg, **({} if capacity is None else {"capacity": capacity}))
    want = D.scene_reference(pkg, oracle, capacity)
    f, h = _pair(pkg, rec, sp, cfg, pool)
    totals = _totals(pool)
    for i in range(D.SCENE_STEPS):
        f.DispatchCompute()
        pool, totals = _host_step(pkg, h, cfg, pool, totals)
        _same_pool(f, pool, totals, f"substep {i}")
        ref_pool, ref_t = want[i]
        assert pool.tobytes() == ref_pool.tobytes(), f"substep {i}: host loop against the numpy reference"
        assert {k: totals[k] for k in ref_t} == ref_t, i
        assert totals["alive"] <= cfg.capacity
    assert_records_equal(f.download(), h.download(), "records with and without a pool")
    assert totals["dropped"] == want[-1][1]["dropped"] > 0
    f.close()
    h.close()


@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 257])
def test_smallest_capacities(pkg, oracle, capacity):
    rec, sp, _, pool = D.scene(pkg, oracle)
    rec = rec[:4001]                                                         # not a multiple of the block
    cfg = _cfg(pkg, capacity=capacity)
    f, h = _pair(pkg, rec, sp, cfg, pool[2:2 + min(capacity, 2)])
    pool = pool[2:2 + min(capacity, 2)]
    totals = _totals(pool)
    for i in range(5):
        f.DispatchCompute()
        pool, totals = _host_step(pkg, h, cfg, pool, totals)
        _same_pool(f, pool, totals, f"C = {capacity}, substep {i}")
    assert totals["alive"] == capacity and totals["dropped"] > 0
    f.close()
    h.close()


@pytest.mark.parametrize("capacity", [4096, 20])
def test_eight_children_at_the_last_id(pkg, oracle, capacity):
    rec, sp, _, _ = D.scene(pkg, oracle)
    rec = rec[:4001].copy()
    rec["padA"] = 0.0
    rec["padA"][[5, 300, 4000]] = 10.0                                       # lambda = 3 * 9.8: eight children each
    cfg = _cfg(pkg, capacity=capacity, maxPerParent=8, maxAge=1.0, lifeMin=0.5, lifeMax=1.0)
    f, h = _pair(pkg, rec, sp, cfg, D.empty())
    pool, totals = _host_step(pkg, h, cfg, D.empty(), _totals(D.empty()))
    f.DispatchCompute()
    _same_pool(f, pool, totals, "first substep")
    assert totals["spawned"] == 24 and list(pool["parent"]) == ([5] * 8 + [300] * 8 + [4000] * 8)[:capacity]
    assert totals["dropped"] == 24 - min(capacity, 24)                       # C = 20: the last parent keeps four of its eight
    for i in range(3):
        f.DispatchCompute()
        pool, totals = _host_step(pkg, h, cfg, pool, totals)
        _same_pool(f, pool, totals, f"substep {i + 1}")
    f.close()
    h.close()


def test_dispatch_n_and_graph_replay_equal_eager_dispatches(pkg, oracle):
    rec, sp, _, pool = D.scene(pkg, oracle)
    cfg = _cfg(pkg)
    eager = engine(pkg, rec, sp)
    plain = engine(pkg, rec, sp)                                             # sph_dispatch_n without graphs
    graph = engine(pkg, rec, sp, graph=1)                                    # call 1 eager, call 2 captured, calls 3 .. replayed
    for f in (eager, plain, graph):
        f.set_diffuse(cfg)
        f.seed_diffuse(pool)
    shots = []
    for _ in range(2):
        for _ in range(16):
            eager.DispatchCompute()
        shots.append((eager.diffuse(), eager.diffuse_info(), eager.download()))
    for f, what in ((plain, "sph_dispatch_n"), (graph, "captured and replayed")):
        for want_pool, want_info, want_rec in shots:
            f.DispatchN(8)
            f.DispatchN(8)
            assert f.diffuse().tobytes() == want_pool.tobytes(), what
            assert f.diffuse_info() == want_info, what
            assert_records_equal(f.download(), want_rec, what)
    launches = graph.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
    assert plain.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == 0 and launches >= 2     # the captured call and at least one replay
    assert want_info["substeps"] == 32 and want_info["spawned"] > 0 and all(p != 0 for p in graph.diffuse_device())
    # a coefficient changed between two replays takes effect, with no new capture
    other = _cfg(pkg, rate=1500.0, sprayBelow=3, kd=0.25)
    for f in (eager, graph):
        f.set_diffuse(other)
    for _ in range(8):
        eager.DispatchCompute()
    graph.DispatchN(8)
    assert graph.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches + 1
    assert graph.diffuse().tobytes() == eager.diffuse().tobytes() and graph.diffuse_info() == eager.diffuse_info()
    plain.DispatchN(8)                                                       # (the old coefficients: another pool)
    assert plain.diffuse_info()["spawned"] != eager.diffuse_info()["spawned"]
    for f in (eager, plain, graph):
        f.close()


def test_fluid_untouched_and_launch_counts_without_a_pool(pkg, oracle):
    rec, sp, _, pool = D.scene(pkg, oracle)
    never, cleared, used = engine(pkg, rec, sp), engine(pkg, rec, sp), engine(pkg, rec, sp)
    for f in (never, cleared, used):
        f.set_option(pkg.SPH_OPT_TIMING, 1)
    cleared.set_diffuse(_cfg(pkg))
    cleared.seed_diffuse(pool)
    cleared.clear_diffuse()
    used.set_diffuse(_cfg(pkg))
    used.seed_diffuse(pool)
    for f in (never, cleared, used):
        f.DispatchCompute()
        f.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
        f.DispatchN(5)
    want = never.download()
    assert cleared.download().tobytes() == want.tobytes() and used.download().tobytes() == want.tobytes()
    counts = [[f.kernel_times()[k][1] for k in pkg.KERNEL_CLASSES] for f in (never, cleared, used)]
    print("launches per class (never set, set and cleared, set):", counts)
    assert counts[0] == counts[1]                                            # with no pool set a dispatch launches what it launched before
    other = pkg.KERNEL_CLASSES.index("other")
    assert counts[2][:other] == counts[0][:other] and counts[2][other] == counts[0][other] + 6      # one timed bracket per substep
    assert cleared.diffuse_config().capacity == 0 and len(cleared.diffuse()) == 0 and cleared.diffuse_info()["substeps"] == 0
    # SPH_OPT_DIFFUSE_TIMED moves the bracket, not the launches: the same pool, still one bracket per substep
    want_pool = used.diffuse()
    for mode in (1, 2):
        g = engine(pkg, rec, sp)
        g.set_option(pkg.SPH_OPT_TIMING, 1)
        g.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, mode)
        assert g.get_option(pkg.SPH_OPT_DIFFUSE_TIMED) == mode
        g.set_diffuse(_cfg(pkg))
        g.seed_diffuse(pool)
        g.DispatchCompute()
        g.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
        g.DispatchN(5)
        assert g.diffuse().tobytes() == want_pool.tobytes() and g.kernel_times()["other"][1] == counts[2][other], mode
        with pytest.raises(pkg.SphError, match="-1"):
            g.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, 3)
        g.close()
    for f in (never, cleared, used):
        f.close()


def _run(pkg, f, h, cfg, pool, totals, n, dt=-1.0, what=""):
    for i in range(n):
        f.DispatchCompute(dt)
        pool, totals = _host_step(pkg, h, cfg, pool, totals, dt)
        _same_pool(f, pool, totals, f"{what}: substep {i}")
    return pool, totals


def test_calls_that_must_not_disturb_the_pool(pkg, oracle):
    rec, sp, _, pool0 = D.scene(pkg, oracle)
    cfg = _cfg(pkg)
    # pause, overrideDt, upload, sph_set_params, impulses between substeps: one run
    f, h = _pair(pkg, rec, sp, cfg, pool0)
    pool, totals = _run(pkg, f, h, cfg, pool0, _totals(pool0), 3, what="plain")
    before, info = f.diffuse(), f.diffuse_info()
    for e in (f, h):
        e.param_pause = 1
    f.DispatchCompute()
    f.DispatchN(4)
    assert f.diffuse().tobytes() == before.tobytes() and f.diffuse_info() == info      # nothing happens, the counter stands
    for e in (f, h):
        e.param_pause = 0
    odt = float(F(0.6) * F(sp.param_timeStep))
    pool, totals = _run(pkg, f, h, cfg, pool, totals, 3, dt=odt, what="overrideDt")
    mid = f.download()
    for e in (f, h):
        e.upload(mid)
    assert f.diffuse().tobytes() == pool.tobytes()
    pool, totals = _run(pkg, f, h, cfg, pool, totals, 2, what="after an upload")
    for e in (f, h):
        e.param_viscosity = 5.0
        e.param_gravityY = -500.0                                            # (the spray's g is the params' gravity)
    pool, totals = _run(pkg, f, h, cfg, pool, totals, 2, what="after sph_set_params")
    for k in range(3):
        for e in (f, h):
            e.ApplyWaveImpulse(20.0, 1.5, 0.1 * k, (0.0, 1.0, 0.0))
            e.ApplyVortexImpulse(3.0, 1.0)
        assert f.diffuse().tobytes() == pool.tobytes()
        pool, totals = _run(pkg, f, h, cfg, pool, totals, 1, what=f"impulse {k}")
    assert_records_equal(f.download(), h.download(), "records")
    assert totals["spawned"] > 500 and min(totals["aliveByKind"]) > 0
    f.close()
    h.close()
    # fountain mode: the pool sees the entry state, before the recycle of the same dispatch
    f, h = _pair(pkg, rec, sp, cfg, pool0)
    for e in (f, h):
        e.fountainMode = 1
        e.fountainOffset = (0.0, -1.0, 0.0)
        e.fountainDrainPerSec = 200.0
        e.fountainDrainLevel = 1.5
    pool, totals = _run(pkg, f, h, cfg, pool0, _totals(pool0), 5, what="fountain")
    assert f.fountainSeed == 5 and totals["spawned"] > 0
    assert_records_equal(f.download(), h.download(), "fountain mode")
    f.close()
    h.close()
    # river mode
    import test_gpu_river
    P, rsp, _, river, _, heights = test_gpu_river._scene(pkg, oracle)
    P = oracle.substep_river(P, to_oracle_params(oracle, rsp), oracle.ORiver.from_buffer_copy(bytes(river)), heights, steps=2)   # densities
    P["padA"][::8] = 0.9
    f, h = _pair(pkg, P, rsp, cfg, D.empty())
    for e in (f, h):
        e.set_river(river, heights)
    pool, totals = _run(pkg, f, h, cfg, D.empty(), _totals(D.empty()), 5, what="river")
    assert totals["spawned"] > 0
    assert_records_equal(f.download(), h.download(), "river mode")
    f.close()
    h.close()


def test_lifetimes(pkg, oracle):
    rec, sp, _, pool0 = D.scene(pkg, oracle)
    cfg = _cfg(pkg, rate=0.0)                                                # no spawning: only the seeded records
    f = engine(pkg, rec, sp)
    f.set_diffuse(cfg)
    g = pkg.compute_grid_extents(sp)
    hi = [g.gridMin[a] + g.dims[a] * g.cellSize for a in range(3)]
    bad = np.zeros(8, pkg.DIFFUSE_DTYPE)
    bad["life"] = 1.0
    bad["pos"][0] = (np.nan, 0, 0)
    bad["pos"][1] = (0, np.inf, 0)
    bad["pos"][2] = (0, 0, -np.inf)
    bad["pos"][3] = (0.0, 2.1, 0.0)                                          # spray above the fluid, a finite position ...
    bad["vel"][3] = (np.inf, 0, 0)                                           # ... that the move makes non-finite
    bad["pos"][4] = (hi[0] + 1.0, 0, 0)
    bad["pos"][5] = (0, g.gridMin[1] - 1.0, 0)
    bad["pos"][6] = (0, 0, hi[2] + 50.0)
    bad["pos"][7] = (0.1, 0.2, 0.3)                                          # the one that lives
    f.seed_diffuse(bad)
    assert f.diffuse_info()["alive"] == 8 and f.diffuse().tobytes() == bad.tobytes()
    f.DispatchCompute()
    info = f.diffuse_info()
    assert (info["nonFinite"], info["leftBox"], info["diedLife"], info["diedAge"], info["alive"], info["seeded"]) == (4, 3, 0, 0, 1, 8), info
    left = f.diffuse()
    assert len(left) == 1 and left["age"][0] == F(sp.param_timeStep) and np.isfinite(left["pos"]).all()
    with pytest.raises(pkg.SphError, match="-4"):
        f.seed_diffuse(np.zeros(cfg.capacity, pkg.DIFFUSE_DTYPE))            # alive + m > capacity: nothing written
    assert f.diffuse().tobytes() == left.tobytes()
    # sph_reset drops the pool
    f.ResetSimulation(seed=3)
    assert f.diffuse_config().capacity == 0 and len(f.diffuse()) == 0 and f.diffuse_device() == (0, 0)
    assert f.diffuse_info()["alive"] == 0 and f.diffuse_info()["substeps"] == 0
    with pytest.raises(pkg.SphError, match="-3"):
        f.seed_diffuse(bad)
    f.DispatchN(2)
    f.set_diffuse(cfg)                                                       # and a new pool starts from nothing
    f.DispatchCompute()
    assert f.diffuse_info()["substeps"] == 1
    f.close()


BAD = (dict(rate=np.nan), dict(rate=-1.0), dict(lifeMin=np.inf), dict(lifeMin=-0.1), dict(lifeMax=np.nan), dict(spread=-1.0), dict(spread=np.inf),
       dict(lifeMin=0.5, lifeMax=0.25), dict(maxPerParent=0), dict(maxPerParent=9), dict(sprayBelow=7, bubbleAbove=6), dict(kd=-0.01),
       dict(kd=1.01), dict(kd=np.nan), dict(capacity=2 ** 31))


def test_refusals_and_re_set(pkg, oracle):
    L = pkg.load_library()
    rec, sp, _, pool0 = D.scene(pkg, oracle)
    cfg = _cfg(pkg)
    # a z-slab engine: refused before anything is allocated
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    assert L.sph_diffuse_set(slab._h, C.byref(cfg)) == -3 and b"slab" in L.sph_last_error()
    got = pkg.SphDiffuseConfig()
    assert L.sph_diffuse_get(slab._h, C.byref(got)) == 0 and got.capacity == 0
    slab.close()
    f, h = engine(pkg, rec, sp), engine(pkg, rec, sp)
    # SPH_OPT_GRID_BUILD 1: at set ...
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.set_diffuse(cfg)
    assert f.diffuse_config().capacity == 0 and f.diffuse_device() == (0, 0)
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    f.set_diffuse(cfg)
    f.seed_diffuse(pool0)
    pool, totals = _run(pkg, f, h, cfg, pool0, _totals(pool0), 2, what="before the refusals")
    rec_a = f.download()
    # ... and at dispatch: refused, nothing changes
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="-3"):
        f.DispatchN(3)
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    _same_pool(f, pool, totals, "after the refused dispatches")
    assert_records_equal(f.download(), rec_a, "after the refused dispatches")
    # bad configs: SPH_ERR_ARG, the previous config stays in force
    for bad in BAD:
        with pytest.raises(pkg.SphError, match="-1"):
            f.set_diffuse(_cfg(pkg, **bad))
        assert bytes(f.diffuse_config()) == bytes(cfg), bad
    pool, totals = _run(pkg, f, h, cfg, pool, totals, 2, what="after the refused configs")
    # set twice: the same capacity keeps the pool and replaces the coefficients ...
    cfg2 = _cfg(pkg, rate=500.0, bubbleAbove=9)
    f.set_diffuse(cfg2)
    _same_pool(f, pool, totals, "set with the same capacity")
    pool, totals = _run(pkg, f, h, cfg2, pool, totals, 2, what="new coefficients")
    # ... another capacity starts a new, empty pool
    cfg3 = _cfg(pkg, capacity=300)
    f.set_diffuse(cfg3)
    assert f.diffuse_info()["alive"] == 0 and f.diffuse_info()["substeps"] == 0 and f.diffuse_info()["capacity"] == 300
    pool, totals = _run(pkg, f, h, cfg3, D.empty(), _totals(D.empty()), 2, what="a new capacity")
    # clear, then set again
    f.clear_diffuse()
    assert f.diffuse_config().capacity == 0 and len(f.diffuse()) == 0
    f.DispatchCompute()
    h.DispatchCompute()
    f.set_diffuse(cfg)
    pool, totals = _run(pkg, f, h, cfg, D.empty(), _totals(D.empty()), 2, what="set after clear")
    assert totals["spawned"] > 0
    assert_records_equal(f.download(), h.download(), "records")
    f.close()
    h.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_breaking_wave_example(pkg, tmp_path):
    frames = 5
    res = run_example(build_example(pkg, "breaking_wave", tmp_path), [frames], timeout=300)
    assert res.returncode == 0 and "breaking_wave OK" in res.stdout
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(lines) == frames
    last = {k: int(v) for k, v in (w.split("=") for w in lines[-1].split()[2:])}
    assert last["spray"] > 0 and last["foam"] > 0 and last["bubbles"] > 0    # the defaults make all three classes on the default scene
    # the same run through the Python mirror
    f = pkg.SPHFluidGPU(50000, seed=7)
    f.set_diffuse()
    phase = F(0.0)
    for _ in range(frames):
        f.ApplyWaveImpulse(1.5, 3.0, float(phase), (0.0, 1.0, 0.0))
        phase = F(phase + F(4.0) / F(60.0))
        f.DispatchN(16, float(f.param_timeStep))
    info = f.diffuse_info()
    kinds = np.bincount(f.diffuse()["kind"], minlength=3)
    f.close()
    assert (last["spray"], last["foam"], last["bubbles"]) == tuple(int(x) for x in kinds)
    assert (last["alive"], last["spawned"], last["left_box"]) == (info["alive"], info["spawned"], info["leftBox"])


# ---- random call sequences: diffuse particles mixed with tracers, scalars and obstacles, against the host loop ----
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7]
OPS = ("dispatch", "dispatch", "dispatch", "impulse", "params", "tracers", "scalars", "obstacles", "coefficients", "seed", "pause", "upload")


def _sequence(seed):
    rng = np.random.default_rng(9100 + seed)
    return rng, [str(rng.choice(OPS)) for _ in range(12)] + ["dispatch"]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_call_sequences_against_the_host_loop(pkg, oracle, seed):
    """One drawn sequence on the engine under test (sph_dispatch_n, graphs on for odd seeds, the other record mode for seeds 2, 3, 6, 7)
    and on the host-loop engine, which gets the same calls except the pool's and steps one substep at a time."""
    rec, sp, _, pool = D.scene(pkg, oracle)
    rng, ops = _sequence(seed)
    cfg = _cfg(pkg, capacity=int(rng.choice([200, 1000, 4096])))
    f, h = _pair(pkg, rec, sp, cfg, pool, graph=seed & 1, aos=(seed >> 1) & 1)
    totals = _totals(pool)
    log = []
    try:
        for op in ops:
            log.append(op)
            what = f"seed {seed}: after {log}"
            if op == "dispatch":
                k = int(rng.choice([1, 2, 3, 8, 8]))
                dt = float(rng.choice([-1.0, -1.0, 0.0007]))
                f.DispatchN(k, dt) if k > 1 else f.DispatchCompute(dt)
                for _ in range(k):
                    pool, totals = _host_step(pkg, h, cfg, pool, totals, dt)
            elif op == "impulse":
                for e in (f, h):
                    e.ApplyWaveImpulse(15.0, 1.5, 0.3, (0.0, 1.0, 0.0))
            elif op == "params":
                v = float(rng.choice([2.0, 3.5, 6.0]))
                for e in (f, h):
                    e.param_viscosity = v
            elif op == "tracers":
                pts = rec["pos"][:: int(rng.choice([64, 97])), :3] if rng.random() < 0.8 else np.zeros((0, 3), F)
                for e in (f, h):
                    e.set_tracers(pts, pkg.SPH_TRACER_MIDPOINT) if len(pts) else e.clear_tracers()
            elif op == "scalars":
                for e in (f, h):
                    e.set_scalars(None, diffusivity=0.05)
            elif op == "obstacles":
                body = [pkg.obstacle(pkg.SPH_OBSTACLE_SPHERE, (0.0, -0.5, 0.0), (0.6, 0.0, 0.0), vel=(0.0, 40.0, 0.0))] if rng.random() < 0.8 else []
                for e in (f, h):
                    e.set_obstacles(body)
            elif op == "coefficients":
                cfg = _cfg(pkg, capacity=cfg.capacity, rate=float(rng.choice([0.0, 1000.0, 6000.0])), sprayBelow=int(rng.choice([3, 4, 5])),
                           kd=float(rng.choice([0.0, 0.5, 1.0])), maxPerParent=int(rng.choice([1, 3, 8])))
                f.set_diffuse(cfg)
            elif op == "seed":
                m = min(int(rng.integers(1, 6)), cfg.capacity - len(pool))
                extra = np.zeros(m, pkg.DIFFUSE_DTYPE)
                extra["pos"] = rng.uniform(-2.4, 2.4, (m, 3)).astype(F)      # some of them outside the box
                extra["vel"] = rng.normal(0, 30, (m, 3)).astype(F)
                extra["life"] = rng.uniform(0.0, 0.01, m).astype(F)
                f.seed_diffuse(extra)
                pool = np.concatenate([pool, extra])
                kinds = list(totals.get("aliveByKind", [0, 0, 0]))
                kinds[0] += m                                                # (the records' kind field, as sph_diffuse_seed counts it)
                totals = dict(totals, seeded=totals["seeded"] + m, alive=totals["alive"] + m, aliveByKind=kinds)
            elif op == "pause":
                for e in (f, h):
                    e.param_pause = 1
                f.DispatchN(3)
                h.DispatchCompute()
                for e in (f, h):
                    e.param_pause = 0
            elif op == "upload":
                mid = f.download()
                for e in (f, h):
                    e.upload(mid)
            if totals.get("substeps", 0):
                _same_pool(f, pool, totals, what)
            else:
                assert f.diffuse().tobytes() == pool.tobytes(), what
        assert_records_equal(f.download(), h.download(), f"seed {seed}: records after {log}")
        assert f.num_tracers() == h.num_tracers() and (f.num_tracers() == 0 or f.tracers().tobytes() == h.tracers().tobytes())
        assert f.num_scalar_channels() == h.num_scalar_channels() and (f.num_scalar_channels() == 0 or f.scalars().tobytes() == h.scalars().tobytes())
        assert f.obstacles().tobytes() == h.obstacles().tobytes()
    finally:
        f.close()
        h.close()
