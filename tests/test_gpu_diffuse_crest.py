"""Crest births of the diffuse pool on the GPU (include/sph_abi.h "births at wave crests"): the pool and the
books after every substep against the host loop
    s = sample(pool.pos); P = download(); rows = shell_host(P) (or shell()); dispatch(dt); pool = diffuse_step_host(..., crest, rows)
run on a second engine that holds no pool.  Everything is compared bit for bit, order included; no tolerance is used.  The scene and
its settings are those of tests/test_diffuse_crest_cpu.py, which shows with the numpy restatement that the run contains every event."""
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal
import diffuse_crest_ref as K
import diffuse_ref as D
import query_scenes
from support import build_example, engine, run_example

pytestmark = pytest.mark.gpu

F = np.float32
INFO_KEYS = ("substeps", "spawned", "dropped", "diedLife", "diedAge", "leftBox", "nonFinite", "seeded", "alive", "aliveByKind")


def _cfg(pkg, **kw):
    return pkg.diffuse_config(**dict(D.SCENE_CONFIG, **kw))


def _totals(pool):
    return {"seeded": len(pool), "alive": len(pool)}


def _on(crest):
    return crest is not None and crest.rate != 0


def _host_step(pkg, h, cfg, crest, pool, totals, dt=-1.0, query=False, seen=None):
    """One turn of the host loop on the engine h (which holds no pool).  query: the rows from h.shell() instead of shell_host."""
    s = h.sample(pool["pos"]) if len(pool) else np.zeros(0, pkg.SAMPLE_DTYPE)
    P = h.download()
    rows = None
    if _on(crest):
        fluid_only = bool(crest.flags & pkg.SPH_SHELL_FLUID_ONLY)
        rows = (h.shell(crest.radius if crest.radius > 0 else None, crest.offset, crest.minCount, fluid_only)[0] if query
                else K.shell_rows(pkg, P, h.params, crest))
        if seen is not None:
            step = F(dt) if dt > 0 else F(h.params.param_timeStep)
            seen.append(K.events(P, rows, cfg, crest, step, totals.get("substeps", 0)))
    h.DispatchCompute(dt)
    return pkg.diffuse_step_host(cfg, h.params, pool, s, P, totals.get("substeps", 0), dt=dt, totals=totals, crest=crest if _on(crest) else None,
                                 shell_rows=rows)


def _same(f, pool, totals, what):
    got = f.diffuse()
    assert len(got) == len(pool), f"{what}: {len(got)} records, the host loop has {len(pool)}"
    if got.tobytes() != pool.tobytes():
        for name in got.dtype.names:
            bad = np.nonzero((got[name] != pool[name]) & ~((got[name] != got[name]) & (pool[name] != pool[name])))[0]
            if len(bad):
                raise AssertionError(f"{what}: field {name} differs in {len(bad)} records, first {bad[0]}: {got[name][bad[0]]} vs {pool[name][bad[0]]}")
        raise AssertionError(f"{what}: pools differ")
    info, books = f.diffuse_info(), f.diffuse_crest_info()
    assert {k: info[k] for k in INFO_KEYS} == {k: totals[k] for k in INFO_KEYS}, f"{what}: {info} vs {totals}"
    assert {k: books[k] for k in K.BOOKS} == {k: totals.get(k, 0) for k in K.BOOKS}, f"{what}: {books} vs {totals}"
    gone = sum(info[k] for k in ("dropped", "diedLife", "diedAge", "leftBox", "nonFinite"))
    assert info["alive"] == info["seeded"] + info["spawned"] - gone <= info["capacity"] and books["crestSpawned"] <= info["spawned"], what


def _pair(pkg, rec, sp, cfg, crest, pool, **kw):
    f, h = engine(pkg, rec, sp, **kw), engine(pkg, rec, sp)
    f.set_diffuse(cfg)
    if crest is not None:
        f.set_diffuse_crest(crest)
    f.seed_diffuse(pool)
    return f, h


def _run(pkg, f, h, cfg, crest, pool, totals, n, dt=-1.0, what="", query=False, seen=None):
    for i in range(n):
        f.DispatchCompute(dt)
        pool, totals = _host_step(pkg, h, cfg, crest, pool, totals, dt, query, seen)
        _same(f, pool, totals, f"{what}: substep {i}")
    return pool, totals


@pytest.mark.parametrize("capacity,every,n", [(K.ROOMY, 1, None), (64, 1, None), (K.ROOMY, 3, None), (K.ROOMY, 1, 4001)],
                         ids=["no drops", "small capacity", "every 3", "n 4001"])
def test_pool_equals_the_host_loop(pkg, oracle, capacity, every, n):
    rec, sp, _, pool = D.scene(pkg, oracle)
    rec = rec if n is None else rec[:n].copy()
    cfg = _cfg(pkg, capacity=capacity)
    crest = K.scene_crest(pkg, sp, every=every)
    f, h = _pair(pkg, rec, sp, cfg, crest, pool)
    assert bytes(f.diffuse_crest()) == bytes(crest) and f.diffuse_crest_info()["on"] == 1
    seen = []
    pool, totals = _run(pkg, f, h, cfg, crest, pool, _totals(pool), D.SCENE_STEPS, what=f"C {capacity} every {every} n {n}", seen=seen)
    assert_records_equal(f.download(), h.download(), "records with and without a pool")
    ev = {k: sum(e.get(k, 0) for e in seen) for k in ("crestBorn", "crestOnly", "both", "pc0", "pc1", "pk0", "pk1")}
    print("events:", ev, "books:", {k: totals[k] for k in K.BOOKS}, "spawned", totals["spawned"], "dropped", totals["dropped"])
    assert totals["crestSpawned"] == ev["crestBorn"] > 0 and totals["acting"] == len(range(0, D.SCENE_STEPS, every))
    assert ev["crestOnly"] > 0 and ev["both"] > 0                            # parents of the crest term alone, and of both terms
    assert min(ev["pc0"], ev["pc1"], ev["pk0"], ev["pk1"]) > 0               # both windows clamp at both ends somewhere in the run
    assert (totals["dropped"] > 0) == (capacity == 64)
    assert sum(1 for e in seen if e) == totals["acting"]
    f.close()
    h.close()


def _moving(rec, seed, speed=20.0):
    rec = rec.copy()
    rec["vel"][:, :3] = np.random.default_rng(seed).normal(0.0, speed, (len(rec), 3)).astype(F)
    rec["density"] = 1000.0
    return rec


def test_edge_cases_against_the_host_loop(pkg, oracle):
    rec, sp, _, _ = D.scene(pkg, oracle)
    cfg = _cfg(pkg, capacity=2048)
    h0 = float(sp.param_h)
    # one particle: isolated, a shell member and never a parent (align 0 would let a zero normal pass)
    one = _moving(rec[:1], 1)
    crest = K.scene_crest(pkg, sp, align=0.0, rate=1e6)
    f, h = _pair(pkg, one, sp, cfg, crest, D.empty())
    _, t = _run(pkg, f, h, cfg, crest, D.empty(), _totals(D.empty()), 3, what="n = 1")
    assert (t["acting"], t["crestSpawned"], t["shellSize"]) == (3, 0, 1)
    f.close()
    h.close()
    # an offset no centroid reaches: the shell is empty, the compacted count 0
    crest = K.scene_crest(pkg, sp, offset=10.0)
    f, h = _pair(pkg, rec, sp, cfg, crest, D.empty())
    _, t = _run(pkg, f, h, cfg, crest, D.empty(), _totals(D.empty()), 3, what="empty shell", query=True)
    assert (t["acting"], t["crestSpawned"], t["shellSize"]) == (3, 0, 0) and t["spawned"] > 0
    f.close()
    h.close()
    # a radius below every distance: everybody is isolated, the shell is everybody, nobody qualifies
    crest = K.scene_crest(pkg, sp, radius=1e-4 * h0, align=0.0, rate=1e6)
    f, h = _pair(pkg, rec, sp, cfg, crest, D.empty())
    _, t = _run(pkg, f, h, cfg, crest, D.empty(), _totals(D.empty()), 2, what="all isolated")
    assert (t["acting"], t["crestSpawned"], t["shellSize"]) == (2, 0, len(rec))
    f.close()
    h.close()
    # ghosts of every kind under SPH_SHELL_FLUID_ONLY: never candidates, never members, never parents
    grec, gsp = query_scenes.with_ghosts(pkg)
    grec = _moving(grec, 2)
    gcfg = _cfg(pkg, capacity=4096, maxAge=1.0, lifeMax=1.0)
    crest = pkg.diffuse_crest_config(rate=1e5, radius=0.0, crestMin=0.05, crestMax=1.0, speedMin=5.0, speedMax=30.0, flags=pkg.SPH_SHELL_FLUID_ONLY)
    f, h = _pair(pkg, grec, gsp, gcfg, crest, D.empty())
    pool, t = _run(pkg, f, h, gcfg, crest, D.empty(), _totals(D.empty()), 3, what="ghosts, fluid only", query=True)
    assert t["crestSpawned"] > 0 and not (grec["isGhost"][pool["parent"]] != 0).any() and 0 < t["shellSize"] <= (grec["isGhost"] == 0).sum()
    f.close()
    h.close()


def test_dispatch_n_and_graph_replay_equal_eager_dispatches(pkg, oracle):
    rec, sp, _, pool = D.scene(pkg, oracle)
    cfg = _cfg(pkg, capacity=K.ROOMY)
    crest = K.scene_crest(pkg, sp, every=2)
    eager = engine(pkg, rec, sp)
    plain = engine(pkg, rec, sp)                                             # sph_dispatch_n without graphs
    graph = engine(pkg, rec, sp, graph=1)                                    # eager until the buffers stand, then captured, then replayed
    for f in (eager, plain, graph):
        f.set_diffuse(cfg)
        f.set_diffuse_crest(crest)
        f.seed_diffuse(pool)
    shots = []
    for _ in range(2):
        for _ in range(16):
            eager.DispatchCompute()
        shots.append((eager.diffuse(), eager.diffuse_info(), eager.diffuse_crest_info(), eager.download()))
    for f, what in ((plain, "sph_dispatch_n"), (graph, "captured and replayed")):
        for want_pool, want_info, want_books, want_rec in shots:
            f.DispatchN(8)
            f.DispatchN(8)
            assert f.diffuse().tobytes() == want_pool.tobytes(), what
            assert f.diffuse_info() == want_info and f.diffuse_crest_info() == want_books, what
            assert_records_equal(f.download(), want_rec, what)
    launches = graph.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
    assert plain.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == 0 and launches >= 2     # the captured call and at least one replay
    assert want_books["acting"] == 16 and want_books["crestSpawned"] > 0
    # rate, a window, every: changed between two replays, in force at once, with no new capture
    for change in (dict(rate=9000.0), dict(crestMin=0.5, speedMax=20.0), dict(every=3), dict(every=1, align=0.2)):
        crest = pkg.diffuse_crest_config(**dict({k: getattr(crest, k) for k, _ in crest._fields_ if k != "pad"}, **change))
        before = eager.diffuse_crest_info()["crestSpawned"]
        for f in (eager, graph):
            f.set_diffuse_crest(crest)
        for _ in range(8):
            eager.DispatchCompute()
        graph.DispatchN(8)
        launches += 1
        assert graph.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) == launches, change
        assert graph.diffuse().tobytes() == eager.diffuse().tobytes() and graph.diffuse_info() == eager.diffuse_info(), change
        assert graph.diffuse_crest_info() == eager.diffuse_crest_info() and eager.diffuse_crest_info()["crestSpawned"] > before, change
    plain.DispatchN(8)                                                       # (the old coefficients: other books)
    assert plain.diffuse_crest_info() != eager.diffuse_crest_info()
    # a launch argument (the radius): in force too; it may capture anew
    crest = pkg.diffuse_crest_config(**dict({k: getattr(crest, k) for k, _ in crest._fields_ if k != "pad"}, radius=0.0, offset=0.2))
    for f in (eager, graph):
        f.set_diffuse_crest(crest)
    for _ in range(3):
        for _ in range(8):
            eager.DispatchCompute()
        graph.DispatchN(8)
        assert graph.diffuse().tobytes() == eager.diffuse().tobytes() and graph.diffuse_crest_info() == eager.diffuse_crest_info()
    assert graph.diffuse_crest_info()["radius"] == F(sp.param_h) and graph.diffuse_crest_info()["stencil"] == 1
    assert graph.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) > launches
    assert_records_equal(graph.download(), eager.download(), "records")
    for f in (eager, plain, graph):
        f.close()


def test_off_means_off(pkg, oracle):
    rec, sp, _, pool = D.scene(pkg, oracle)
    cfg, crest = _cfg(pkg), K.scene_crest(pkg, sp)
    never, cleared, zero, used = (engine(pkg, rec, sp) for _ in range(4))
    for f in (never, cleared, zero, used):
        f.set_option(pkg.SPH_OPT_TIMING, 1)
        f.set_diffuse(cfg)
        f.seed_diffuse(pool)
    cleared.set_diffuse_crest(crest)
    cleared.clear_diffuse_crest()
    zero.set_diffuse_crest(crest)
    zero.set_diffuse_crest(crest, rate=0.0)
    used.set_diffuse_crest(crest)
    for f in (never, cleared, zero, used):
        f.DispatchCompute()
        f.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
        f.DispatchN(5)
    counts = [[f.kernel_times()[k][1] for k in pkg.KERNEL_CLASSES] for f in (never, cleared, zero, used)]
    print("launches per class (never set, set and cleared, set and rate 0, set):", counts)
    assert counts[1] == counts[0] and counts[2] == counts[0]                 # with the term off a dispatch launches what it launched before
    want = never.diffuse()
    for f in (cleared, zero):
        assert f.diffuse().tobytes() == want.tobytes() and f.diffuse_info() == never.diffuse_info()
        assert f.download().tobytes() == never.download().tobytes()
        books = f.diffuse_crest_info()
        assert (books["on"], books["acting"], books["crestSpawned"]) == (0, 0, 0) and f.diffuse_crest().rate == 0
    assert counts[3] == counts[0]                                            # the term on: still one timed bracket per substep
    assert used.diffuse_crest_info()["crestSpawned"] > 0 and used.diffuse_crest_info()["acting"] == 6
    assert used.download().tobytes() == never.download().tobytes()           # and the fluid does not notice
    # SPH_OPT_DIFFUSE_TIMED moves the bracket, not the launches; it has no new value
    want_pool = used.diffuse()
    for mode in (1, 2):
        g = engine(pkg, rec, sp)
        g.set_option(pkg.SPH_OPT_TIMING, 1)
        g.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, mode)
        g.set_diffuse(cfg)
        g.set_diffuse_crest(crest)
        g.seed_diffuse(pool)
        g.DispatchCompute()
        g.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
        g.DispatchN(5)
        other = pkg.KERNEL_CLASSES.index("other")
        assert g.diffuse().tobytes() == want_pool.tobytes() and g.kernel_times()["other"][1] == counts[3][other], mode
        with pytest.raises(pkg.SphError, match="-1"):
            g.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, 3)
        g.close()
    for f in (never, cleared, zero, used):
        f.close()


BAD = (dict(rate=np.nan), dict(rate=-1.0), dict(rate=np.inf), dict(radius=np.nan), dict(radius=1e3), dict(offset=-0.1), dict(offset=np.nan),
       dict(crestMin=1.0, crestMax=1.0), dict(crestMin=2.0, crestMax=1.0), dict(crestMax=np.inf), dict(crestMin=np.nan),
       dict(speedMin=5.0, speedMax=5.0), dict(speedMax=np.nan), dict(align=-0.01), dict(align=1.01), dict(align=np.nan), dict(every=0),
       dict(flags=2))


def test_lifetimes_and_refusals(pkg, oracle):
    rec, sp, _, pool0 = D.scene(pkg, oracle)
    cfg, crest = _cfg(pkg), K.scene_crest(pkg, sp)
    f, h = engine(pkg, rec, sp), engine(pkg, rec, sp)
    off = bytes(pkg.SphDiffuseCrest())
    # without a pool: SPH_ERR_STATE, also for switching off; the getters give zeros
    for call in (lambda: f.set_diffuse_crest(crest), f.clear_diffuse_crest):
        with pytest.raises(pkg.SphError, match="-3"):
            call()
    assert bytes(f.diffuse_crest()) == off and f.diffuse_crest_info() == dict(acting=0, crestSpawned=0, shellSize=0, on=0, stencil=0, radius=0.0)
    f.set_diffuse(cfg)
    f.set_diffuse_crest(crest)
    f.seed_diffuse(pool0)
    pool, totals = _run(pkg, f, h, cfg, crest, pool0, _totals(pool0), 2, what="before the refusals")
    # bad configs: SPH_ERR_ARG, the previous state stays in force
    for bad in BAD:
        with pytest.raises(pkg.SphError, match="-1"):
            f.set_diffuse_crest(crest, **bad)
        assert bytes(f.diffuse_crest()) == bytes(crest) and f.diffuse_crest_info()["on"] == 1, bad
    pool, totals = _run(pkg, f, h, cfg, crest, pool, totals, 2, what="after the refused configs")
    # sph_diffuse_set with the capacity in place keeps the term ...
    cfg2 = _cfg(pkg, rate=500.0, bubbleAbove=9)
    f.set_diffuse(cfg2)
    assert bytes(f.diffuse_crest()) == bytes(crest)
    pool, totals = _run(pkg, f, h, cfg2, crest, pool, totals, 2, what="new pool coefficients")
    # ... rate 0 switches it off, the books stay; on again, they go on
    f.set_diffuse_crest(crest, rate=0.0)
    assert bytes(f.diffuse_crest()) == off and f.diffuse_crest_info()["on"] == 0 and f.diffuse_crest_info()["crestSpawned"] == totals["crestSpawned"] > 0
    pool, totals = _run(pkg, f, h, cfg2, None, pool, totals, 2, what="switched off")
    f.set_diffuse_crest(crest, every=2)
    crest2 = K.scene_crest(pkg, sp, every=2)
    pool, totals = _run(pkg, f, h, cfg2, crest2, pool, totals, 3, what="switched on again")
    # ... another capacity drops it with the pool
    cfg3 = _cfg(pkg, capacity=300)
    f.set_diffuse(cfg3)
    assert bytes(f.diffuse_crest()) == off and f.diffuse_crest_info()["on"] == 0 and f.diffuse_crest_info()["acting"] == 0
    pool, totals = _run(pkg, f, h, cfg3, None, D.empty(), _totals(D.empty()), 2, what="a new capacity")
    f.set_diffuse_crest(crest)
    pool, totals = _run(pkg, f, h, cfg3, crest, pool, totals, 2, what="a new capacity, the term set again")
    assert totals["crestSpawned"] > 0 and totals["dropped"] > 0
    # sph_diffuse_set(NULL) and sph_reset drop it
    f.clear_diffuse()
    assert bytes(f.diffuse_crest()) == off and f.diffuse_crest_info()["on"] == 0
    with pytest.raises(pkg.SphError, match="-3"):
        f.set_diffuse_crest(crest)
    f.set_diffuse(cfg)
    f.set_diffuse_crest(crest)
    f.ResetSimulation(seed=3)
    assert bytes(f.diffuse_crest()) == off and f.diffuse_crest_info()["on"] == 0 and f.diffuse_config().capacity == 0
    f.DispatchN(2)
    f.close()
    h.close()
    # a radius that the params' grid stops admitting: the dispatch is refused and changes nothing
    own = type(sp).from_buffer_copy(sp)                                      # (the engine edits the params it is given)
    h0 = float(own.param_h)
    f = engine(pkg, rec, own)
    f.set_diffuse(cfg)
    f.set_diffuse_crest(crest, radius=2.5 * h0)
    f.DispatchCompute()
    before, info, books, state = f.diffuse(), f.diffuse_info(), f.diffuse_crest_info(), f.download()
    f.param_h = 0.5 * h0
    for call in (f.DispatchCompute, lambda: f.DispatchN(3)):
        with pytest.raises(pkg.SphError, match="-3"):
            call()
    f.param_h = h0
    assert f.diffuse().tobytes() == before.tobytes() and f.diffuse_info() == info
    assert {k: f.diffuse_crest_info()[k] for k in K.BOOKS} == {k: books[k] for k in K.BOOKS}
    assert_records_equal(f.download(), state, "after the refused dispatches")
    f.DispatchCompute()
    assert f.diffuse_crest_info()["acting"] == books["acting"] + 1
    f.close()


OPS = ("dispatch", "dispatch", "dispatch", "impulse", "coefficients", "crest", "crest", "seed", "shell", "sample")


def test_mixed_call_sequence_against_the_host_loop(pkg, oracle):
    """One drawn sequence on the engine under test (sph_dispatch_n with graphs on) and on the host-loop engine, which gets the same
    calls except the pool's and steps one substep at a time.  shell() and sample() on the engine under test in between: the query's
    scratch and the in-substep pass's are not each other's."""
    rec, sp, _, pool = D.scene(pkg, oracle)
    rng = np.random.default_rng(2212)
    ops = [str(rng.choice(OPS)) for _ in range(16)] + ["shell", "dispatch", "dispatch"]
    cfg = _cfg(pkg, capacity=3000)
    crest = K.scene_crest(pkg, sp)
    f, h = _pair(pkg, rec, sp, cfg, crest, pool, graph=1)
    totals = _totals(pool)
    log = []
    try:
        for op in ops:
            log.append(op)
            what = f"after {log}"
            if op == "dispatch":
                k = int(rng.choice([1, 2, 4, 4]))
                dt = float(rng.choice([-1.0, -1.0, 0.0007]))
                f.DispatchN(k, dt) if k > 1 else f.DispatchCompute(dt)
                for _ in range(k):
                    pool, totals = _host_step(pkg, h, cfg, crest, pool, totals, dt)
            elif op == "impulse":
                for e in (f, h):
                    e.ApplyWaveImpulse(15.0, 1.5, 0.3, (0.0, 1.0, 0.0))
            elif op == "coefficients":
                cfg = _cfg(pkg, capacity=cfg.capacity, rate=float(rng.choice([0.0, 1000.0, 6000.0])), maxPerParent=int(rng.choice([1, 3, 8])))
                f.set_diffuse(cfg)
            elif op == "crest":
                if rng.random() < 0.2:
                    crest = None
                    f.clear_diffuse_crest()
                else:
                    crest = K.scene_crest(pkg, sp, rate=float(rng.choice([2000.0, 8000.0])), every=int(rng.choice([1, 2, 3])),
                                          radius=float(rng.choice([0.0, 1.5 * sp.param_h, 2.0 * sp.param_h])), crestMin=float(rng.choice([0.1, 0.25])))
                    f.set_diffuse_crest(crest)
            elif op == "seed":
                m = min(int(rng.integers(1, 6)), cfg.capacity - len(pool))
                extra = np.zeros(m, pkg.DIFFUSE_DTYPE)
                extra["pos"] = rng.uniform(-2.4, 2.4, (m, 3)).astype(F)
                extra["vel"] = rng.normal(0, 30, (m, 3)).astype(F)
                extra["life"] = rng.uniform(0.0, 0.01, m).astype(F)
                f.seed_diffuse(extra)
                pool = np.concatenate([pool, extra])
                kinds = list(totals.get("aliveByKind", [0, 0, 0]))
                kinds[0] += m
                totals = dict(totals, seeded=totals["seeded"] + m, alive=totals["alive"] + m, aliveByKind=kinds)
            elif op == "shell":                                              # another radius and more rows than the substep's pass has slots for
                radius = float(rng.choice([1.0, 2.5])) * float(sp.param_h)
                rows, ids = f.shell(radius, 0.05)
                want, want_ids, _ = pkg.shell_host(f.download(), f.params, radius=radius, offset=0.05)
                assert rows.tobytes() == want.tobytes() and ids.tobytes() == want_ids.tobytes(), what
                pts = rng.uniform(-2.0, 2.0, (5000, 3)).astype(F)
                f.query_shell(pts, radius)
            elif op == "sample":
                f.sample(rec["pos"][::7, :3])
            if totals.get("substeps", 0):
                _same(f, pool, totals, what)
            else:
                assert f.diffuse().tobytes() == pool.tobytes(), what
        assert_records_equal(f.download(), h.download(), f"records after {log}")
        assert totals["crestSpawned"] > 0 and f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) >= 1
    finally:
        f.close()
        h.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_crest_spray_example(pkg, tmp_path):
    frames = 3
    res = run_example(build_example(pkg, "crest_spray", tmp_path), [frames], timeout=300)
    assert res.returncode == 0 and "crest_spray OK" in res.stdout
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(lines) == frames
    last = {k: int(v) for k, v in (w.split("=") for w in lines[-1].split()[2:])}
    assert last["acting"] == 16 * frames and last["shell"] > 0 and last["crest_born"] > 0
    assert last["spray"] + last["foam"] + last["bubbles"] == last["alive"]
