"""Active scalars on the GPU (include/sph_abi.h "active scalars").

The identity that needs no oracle: one substep with the coupling off, downloaded, then the host twin sph_scalars_couple_host (which
tests/test_coupling_cpu.py pins to the numpy restatement) must equal one substep with the coupling on, bit for bit in records and
values; the books lie within coupling_ref.books_bound of the correctly rounded sums (the terms are exactly defined, only the order of
their fp64 sum is free).  Under SPH_OPT_GRAPH a call covers at least two substeps, between which nothing can be downloaded: there the
replayed calls must equal the same calls of an eager engine, whose substeps the identity covers."""
import os
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import body_ref as B
import body_scenes as S
import coupling_ref as CR
import obstacle_ref as R
import scalar_ref as SR
from support import G, build_example, engine, fluid_block, records, run_example, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
K = 2


def _scene(pkg):
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    return (rec, sp, *fluid_block(rec))


def _bodies(pkg, sp, c, E):
    """A spinning, drifting kinematic box and a sphere that test code may make dynamic."""
    return pkg.obstacle_array([pkg.obstacle(R.BOX, c + F(0.15 * E) * np.array([1, 0, -1], F), (0.14 * E, 0.09 * E, 0.11 * E), rotation=(0.8, 0.3, -0.4, 0.2),
                                            vel=(0.4, 0.0, -0.2), omega=(0.0, 3.0, 1.0)),
                               pkg.obstacle(R.SPHERE, c - F(0.2 * E) * np.array([1, 1, 0], F), 0.11 * E)])


def _sources(pkg, c, E):
    """A heater slab (RELAX, world box), a sphere that adds (RATE, world), a source on the spinning box and one on the sphere (body
    frames), the first two overlapping on channel 0."""
    return [pkg.scalar_source(pkg.SPH_SOURCE_BOX, c - F(0.3 * E) * np.array([0, 1, 0], F), (0.6 * E, 0.12 * E, 0.6 * E), channel=0,
                              mode=pkg.SPH_SOURCE_RELAX, rate=60.0, target=2.5),
            pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.35 * E, channel=0, mode=pkg.SPH_SOURCE_RATE, rate=5.0),
            pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.04 * E, 0.0), (0.24 * E, 0.2 * E, 0.2 * E), channel=1, mode=pkg.SPH_SOURCE_RATE, rate=9.0, body=0),
            pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, (0.02 * E, 0.0, 0.0), 0.22 * E, channel=1, mode=pkg.SPH_SOURCE_RELAX, rate=2000.0, target=-0.5, body=1)]


BETA, REF = np.array([0.6, -0.3], F), np.array([0.2, 0.1], F)


def _values(n, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, (n, K)).astype(F)


def _diffusivity(pkg, rec, sp):
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0)
    return F(0.4 / float(s1)) if s1 > 0 else F(0.0)


def _engine(pkg, rec, sp, values, D, aos=1, graph=0, bodies=None, sources=None, beta=None, ref=None, kern=3):
    f = engine(pkg, rec, sp, kern, aos, graph)
    f.set_scalars(values, diffusivity=D, decay=0.0)
    if bodies is not None and len(bodies):
        f.set_obstacles(bodies)
    if sources is not None:
        f.set_scalar_sources(sources)
    if beta is not None:
        f.set_scalar_buoyancy(beta, ref)
    return f


def _check_books(got, books, what, steps=1, dt=None):
    sums, hits, t, n = got
    bound = CR.books_bound(books["hits"], books["abs_sum"])
    err = np.abs(sums - books["sums"])
    print(f"{what}: hits {books['hits'].tolist()} sums {sums.tolist()} max err {err.max() if len(err) else 0:.3g} max bound {bound.max() if len(bound) else 0:.3g}")
    assert hits.tolist() == books["hits"].tolist(), what
    assert (err <= bound).all(), f"{what}: |engine - reference| {err} above {bound}"
    assert n == steps, what
    if dt is not None:
        assert t == float(np.float64(dt) * steps) or steps != 1, what


def _identity(pkg, rec, sp, values, D, bodies, sources, beta, ref, aos, what, need_hits=True):
    """One substep with the coupling off + the host twin against one substep with the coupling on."""
    off = _engine(pkg, rec, sp, values, D, aos, bodies=bodies)
    off.DispatchCompute()
    rec1, c1, poses = off.download(), off.scalars(), off.obstacles()
    off.close()
    want_rec, want_c, sums, hits = pkg.scalars_couple_host(rec1, sp, c1, beta=beta, ref=ref, sources=sources, obstacles=poses)
    on = _engine(pkg, rec, sp, values, D, aos, bodies=bodies, sources=sources, beta=beta, ref=ref)
    on.DispatchCompute()
    got_rec, got_c, got = on.download(), on.scalars(), on.scalar_injected()
    same_bits(on.obstacles(), poses, what + ": the coupling does not touch the bodies")
    on.close()
    assert_records_equal(got_rec, want_rec, what)
    same_bits(got_c, want_c, what + ": values")
    sa = pkg.source_array(sources).view(CR.SOURCE_DTYPE)
    _, _, books = CR.couple(rec1, c1, F(sp.param_timeStep), (sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ), sources=sa,
                            bodies=R.bodies(poses, normalise=False))
    assert hits.tolist() == books["hits"].tolist()
    _check_books(got, books, what, 1 if len(sources) else 0, sp.param_timeStep if len(sources) else None)
    if need_hits:
        assert (books["hits"] > 0).all() and (want_rec["vel"] != rec1["vel"]).any() and (want_c != c1).any(), what
    return got_rec, got_c


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("aos", [0, 1])
def test_identity_with_the_host_twin(pkg, aos, graph):
    rec, sp, c, E = _scene(pkg)
    values, D = _values(len(rec)), _diffusivity(pkg, rec, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)
    if not graph:
        _identity(pkg, rec, sp, values, D, bodies, sources, BETA, REF, aos, f"aos {aos}")
        _identity(pkg, rec, sp, values, D, bodies, sources, None, None, aos, f"aos {aos}, sources alone", need_hits=False)
        _identity(pkg, rec, sp, values, D, bodies, [], BETA, REF, aos, f"aos {aos}, buoyancy alone", need_hits=False)
        return
    runs = []
    for g in (0, 1):
        f = _engine(pkg, rec, sp, values, D, aos, g, bodies=bodies, sources=sources, beta=BETA, ref=REF)
        for _ in range(5):                                               # seen, captured and launched, then replayed
            f.DispatchN(2)
        runs.append((f.download(), f.scalars(), f.obstacles(), f.scalar_injected(), f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)))
        f.close()
    (e_rec, e_c, e_obs, e_inj, e_launches), (g_rec, g_c, g_obs, g_inj, g_launches) = runs
    assert e_launches == 0 and g_launches >= 2                           # captured once, then replayed
    assert_records_equal(g_rec, e_rec, f"aos {aos}: graph replay against eager dispatch")
    same_bits(g_c, e_c, "values under graph replay")
    same_bits(g_obs, e_obs, "poses under graph replay")
    assert g_inj[1].tolist() == e_inj[1].tolist() and (g_inj[1] > 0).all()
    same_bits(g_inj[0], e_inj[0], "books under graph replay (the same kernels in the same order)")
    assert g_inj[2:] == e_inj[2:] and g_inj[3] == 10                     # the substep count advances by the substeps issued, replays included


def test_ten_substeps_against_the_restatement(pkg, oracle):
    """One step ahead: before each substep the device's own state is downloaded; after it the records, values and poses must equal
    oracle substep + scalar_ref.step32 + obstacle_ref.apply + body_ref.step_all (fed with the device's own impulse sums) +
    coupling_ref.couple, bit for bit, and the books must lie within the order bound."""
    rec0, sp, c, E = _scene(pkg)
    op = to_oracle_params(oracle, sp)
    W = S.world_of(pkg, sp)
    dt = F(sp.param_timeStep)
    g = (sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ)
    values, D = _values(len(rec0)), _diffusivity(pkg, rec0, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)
    dyn = [None, pkg.dynamics_sphere(0.6 * float(sp.param_restDensity), 0.11 * E)]
    ds = [B.record(x) for x in pkg.dynamics_array(dyn)]
    sa = pkg.source_array(sources).view(CR.SOURCE_DTYPE)
    f = _engine(pkg, rec0, sp, values, D, bodies=bodies, sources=sources, beta=BETA, ref=REF)
    f.set_obstacle_dynamics(1, dyn[1])
    total = np.zeros(len(sources), np.uint64)
    for k in range(10):
        what = f"substep {k}"
        rec, poses, cur = f.download(), f.obstacles(), f.scalars()
        f.DispatchCompute()
        J, _, _ = f.obstacle_impulses(reset=True)
        b = oracle.build_grid(rec, op)
        diffused, _ = SR.step32(rec, cur, sp.param_h, sp.param_mass, D, 0.0, dt, b["grid"], b["cell_start"], b["order"])
        bs = R.bodies(poses, normalise=False)
        after, want_imp, info = R.apply(bs, F(op.mass), oracle.substep(rec, op, dt=-1.0))
        assert (np.abs(J - want_imp) <= R.impulse_bound(info)).all(), what
        moved = B.step_all(bs, ds, J, W, dt)
        same_bits(f.obstacles(), R.to_array(moved), what + ": poses")
        want_rec, want_c, books = CR.couple(after, diffused, dt, g, beta=BETA, ref=REF, sources=sa, bodies=moved)
        assert_records_equal(f.download(), want_rec, what)
        same_bits(f.scalars(), want_c, what + ": values")
        _check_books(f.scalar_injected(reset=True), books, what, 1, dt)
        total += books["hits"]
    f.close()
    assert (total > 50).all(), total


def _lattice(pkg, n, seed=3):
    """n particles at rest density on a jittered lattice around the origin, in a box that holds them, with two small bodies."""
    side = max(int(np.ceil(n ** (1.0 / 3.0))), 1)
    sp = pkg.default_params(param_boxHalf=(2.0, 2.0, 2.0), param_boxCenter=(0.0, 0.0, 0.0), param_boxEulerDeg=(0.0, 0.0, 0.0))
    s = F(0.85) * F(sp.param_h)
    idx = np.arange(n)
    ijk = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1).astype(F)
    rng = np.random.default_rng(seed + n)
    pos = ((ijk - F(side - 1) / F(2)) * s + rng.uniform(-0.05, 0.05, (n, 3)).astype(F) * s).astype(F)
    rec = records(pkg, pos, rng.uniform(-1.0, 1.0, (n, 3)).astype(F))
    rec["isActive"] = 1
    sp.param_mass = float(F(1000.0) * s * s * s)
    E = float(side * s)
    c = np.zeros(3, F)
    bodies = pkg.obstacle_array([pkg.obstacle(R.BOX, (0.3 * E, 0.0, 0.0), (0.2 * E + 0.1, 0.15 * E + 0.1, 0.2 * E + 0.1), rotation=(0.9, 0.1, 0.3, -0.2), omega=(1.0, 2.0, 0.0)),
                                 pkg.obstacle(R.SPHERE, (-0.3 * E, 0.1 * E, 0.0), 0.1 * E + 0.05)])
    sources = [pkg.scalar_source(pkg.SPH_SOURCE_BOX, c, (E + 1.0, E + 1.0, E + 1.0), channel=0, mode=pkg.SPH_SOURCE_RATE, rate=3.0),
               pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.4 * E + 0.2, channel=1, mode=pkg.SPH_SOURCE_RELAX, rate=300.0, target=1.5),
               pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.0, 0.0), (0.4 * E + 0.3, 0.4 * E + 0.3, 0.4 * E + 0.3), channel=1, mode=pkg.SPH_SOURCE_RATE, rate=7.0, body=0),
               pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, (0.0, 0.0, 0.0), 0.3 * E + 0.3, channel=0, mode=pkg.SPH_SOURCE_RELAX, rate=50.0, target=-2.0, body=1)]
    return rec, sp, bodies, sources


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025])
def test_edge_sizes(pkg, n):
    """Nothing, one lane, one wave more or less, more than a block, one past a sweep of 1024 slots."""
    rec, sp, bodies, sources = _lattice(pkg, n)
    if n == 65:
        rec["isGhost"][::9] = 1
        rec["pos"][5, 1] = np.nan
    values = _values(n, 17)
    D = _diffusivity(pkg, rec, sp) if n else F(0.0)
    got_rec, got_c = _identity(pkg, rec, sp, values, D, bodies, sources, BETA, REF, 1, f"n={n}", need_hits=False)
    assert len(got_rec) == n and got_c.shape == (n, K)
    if n:
        assert (got_c[:, 0] != values[:, 0]).any()                         # the world box holds every particle


def test_second_grid_stride_sweep(pkg):
    """1 048 576 + 1000 particles: the fixed grid of 1024 blocks covers 1 048 576 slots in one sweep, the last 1000 slots (the cells with
    the highest z) are reached only by the grid-stride loop's second pass."""
    n = 1024 * 1024 + 1000
    rec, sp = small_scene(pkg, n=n, grid=96, seed=9)
    rec = rec.copy()
    rec["density"] = 1000.0
    rec["isActive"] = 1
    values = _values(n, 23)
    top = float(rec["pos"][:, 2].max())
    sources = [pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.0, 0.0), (50.0, 50.0, 50.0), channel=0, mode=pkg.SPH_SOURCE_RATE, rate=3.0),
               pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.0, top), (50.0, 50.0, 0.6), channel=1, mode=pkg.SPH_SOURCE_RELAX, rate=100.0, target=4.0)]
    got_rec, got_c = _identity(pkg, rec, sp, values, F(0.0), None, sources, BETA, REF, 1, "two sweeps")
    assert (got_c[:, 0] != values[:, 0]).all()                             # every slot was reached, the second pass included


def test_graph_replay_sees_later_set_calls(pkg):
    rec, sp, c, E = _scene(pkg)
    values, D = _values(len(rec)), _diffusivity(pkg, rec, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)

    def run(graph):
        f = _engine(pkg, rec, sp, values, D, 1, graph, bodies=bodies, sources=sources, beta=BETA, ref=REF)
        for _ in range(4):                                               # (by now the call has been captured and replayed)
            f.DispatchN(2)
        before = f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
        assert before == (2 if graph else 0)
        f.set_scalar_buoyancy(BETA * F(-0.5), REF + F(0.25))
        f.DispatchN(2)
        f.set_scalar_sources(sources[1:3])                               # another count (the books restart)
        f.DispatchN(2)
        f.set_obstacle_motion(0, (-0.3, 0.1, 0.0), (2.0, 0.0, -1.0))
        f.DispatchN(2)
        out = (f.download(), f.scalars(), f.obstacles(), f.scalar_injected(), f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) - before)
        f.close()
        return out

    e, g = run(0), run(1)
    assert e[4] == 0 and g[4] == 3, "three replays, no recapture"
    assert_records_equal(g[0], e[0], "records after the set calls")
    same_bits(g[1], e[1], "values after the set calls")
    same_bits(g[2], e[2], "poses after set_obstacle_motion")
    assert g[3][1].tolist() == e[3][1].tolist() and len(g[3][1]) == 2 and (g[3][1] > 0).all()
    same_bits(g[3][0], e[3][0], "books after the set calls")
    assert g[3][3] == e[3][3] == 4                                        # the books restarted with the other count: two calls of two substeps
    # the changes did take effect: the same calls without them end elsewhere
    f = _engine(pkg, rec, sp, values, D, 1, 1, bodies=bodies, sources=sources, beta=BETA, ref=REF)
    for _ in range(7):
        f.DispatchN(2)
    assert f.download().tobytes() != g[0].tobytes() and f.scalars().tobytes() != g[1].tobytes()
    f.close()


def test_no_side_effects(pkg):
    rec, sp, c, E = _scene(pkg)
    values, D = _values(len(rec)), _diffusivity(pkg, rec, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)
    for aos, with_bodies in ((0, True), (1, True), (0, False)):          # (without bodies and under SPH_OPT_AOS_MODE 0 the pass keeps the 80-byte array current)
        runs = []
        for mode in ("no scalars", "sources"):
            f = engine(pkg, rec, sp, 3, aos, 0)
            if with_bodies:
                f.set_obstacles(bodies)
            if mode == "sources":
                f.set_scalars(values, diffusivity=D)
                f.set_scalar_sources(sources if with_bodies else sources[:2])
            f.DispatchN(3)
            mid = f.download()
            f.DispatchCompute()
            runs.append((mid, f.download(), f.obstacles()))
            if mode == "sources":
                assert (f.scalar_injected()[1] > 0).all() and f.scalar_injected()[3] == 4
            f.close()
        assert_records_equal(runs[1][0], runs[0][0], f"aos {aos}: sources alone, records after 3 substeps")
        assert_records_equal(runs[1][1], runs[0][1], f"aos {aos}: sources alone, records after 4 substeps")
        same_bits(runs[1][2], runs[0][2], "poses")
    # with nothing set, a dispatch launches what it launched with scalars alone: one timed bracket of class "other" per substep
    counts = []
    for mode in ("never set", "set and cleared", "sources", "buoyancy"):
        f = engine(pkg, rec, sp)
        f.set_option(pkg.SPH_OPT_TIMING, 1)
        f.set_scalars(values, diffusivity=D)
        if mode != "never set":
            f.set_scalar_sources(sources[:2])
            f.set_scalar_buoyancy(BETA, REF)
        if mode == "set and cleared":
            f.set_scalar_sources([])
            f.set_scalar_buoyancy(None)
            assert len(f.scalar_sources()) == 0 and not f.scalar_buoyancy()[0].any()
        if mode == "sources":
            f.set_scalar_buoyancy((0.0, 0.0), (1.0, 1.0))                 # zero coefficients are "off" too
        if mode == "buoyancy":
            f.set_scalar_sources([])
        f.DispatchN(5)
        counts.append({k: v[1] for k, v in f.kernel_times().items()})
        f.close()
    assert counts[0] == counts[1], counts[:2]
    print(counts)
    assert counts[2]["other"] == counts[0]["other"] + 5 and counts[3]["other"] == counts[0]["other"] + 5, counts   # one more bracket per substep
    assert {k: v for k, v in counts[2].items() if k != "other"} == {k: v for k, v in counts[0].items() if k != "other"}


def test_books_balance_the_moments(pkg, oracle):
    """With diffusion on and decay 0 the sum of a channel changes by what the sources injected, up to two derived bounds: the rounding of
    the diffusion's own arithmetic (scalar_ref.rounding_bound of every substep, from the float64 evaluation on the state the substep
    started from) and the order bound of the books plus that of the two moment sums (fp64 sums of n values: (n - 1) 2^-53 sum |c|)."""
    rec, sp, c, E = _scene(pkg)
    op = to_oracle_params(oracle, sp)
    values, D = _values(len(rec)), _diffusivity(pkg, rec, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)
    dt = F(sp.param_timeStep)
    g = (sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ)
    sa = pkg.source_array(sources).view(CR.SOURCE_DTYPE)
    f = _engine(pkg, rec, sp, values, D, bodies=bodies, sources=sources, beta=BETA, ref=REF)
    first = f.scalar_moments()
    tgt = SR.targets(rec)
    diffusion = np.zeros(K)
    hits, abs_sum = np.zeros(len(sources)), np.zeros(len(sources))
    N = 6
    for _ in range(N):
        now, cur = f.download(), f.scalars()
        b = oracle.build_grid(now, op)
        ref64 = SR.step64(now, cur, sp.param_h, sp.param_mass, D, 0.0, dt, b["grid"], b["cell_start"], b["order"])
        diffusion += SR.rounding_bound(ref64, cur).sum(axis=0)
        f.DispatchCompute()
        # the terms of this substep's books, from the restatement on the state the coupling step saw (the values before it are not kept
        # by the engine: the diffused values of the twin stand in for them, bit-equal by tests/test_gpu_scalars.py)
        diffused, _ = pkg.scalars_step_host(now, sp, cur, diffusivity=D, decay=0.0)
        after = f.download()
        _, _, books = CR.couple(after, diffused, dt, g, sources=sa, bodies=R.bodies(f.obstacles(), normalise=False))
        hits += books["hits"]
        abs_sum += books["abs_sum"]
    last = f.scalar_moments()
    sums, got_hits, t, n = f.scalar_injected()
    f.close()
    assert n == N and got_hits.tolist() == hits.astype(np.uint64).tolist()
    cnt = int(tgt.sum())
    for k in range(K):
        injected = sum(sums[i] for i in range(len(sources)) if int(sa[i]["channel"]) == k)
        order = sum(CR.books_bound(hits[i:i + 1], abs_sum[i:i + 1])[0] for i in range(len(sources)) if int(sa[i]["channel"]) == k)
        moments = (cnt - 1) * 2.0 ** -53 * (_abs_sum(first[k], cnt) + _abs_sum(last[k], cnt))
        balance = last[k].sum - (first[k].sum + injected)
        print(f"channel {k}: sum {first[k].sum:.9g} -> {last[k].sum:.9g}, injected {injected:.9g}, balance {balance:.3g}, "
              f"diffusion bound {diffusion[k]:.3g}, order bound {order + moments:.3g}")
        assert first[k].count == last[k].count == cnt
        assert abs(injected) > 1.0
        assert abs(balance) <= diffusion[k] + order + moments


def _abs_sum(m, cnt):
    """An upper bound of sum |c| from the moments: sqrt(n sum c^2) (Cauchy-Schwarz)."""
    return float(np.sqrt(cnt * m.sum_squares))


def test_dangling_body_fails_the_dispatch_and_changes_nothing(pkg):
    rec, sp, c, E = _scene(pkg)
    values, D = _values(len(rec)), _diffusivity(pkg, rec, sp)
    bodies, sources = _bodies(pkg, sp, c, E), _sources(pkg, c, E)
    for graph in (0, 1):
        f = _engine(pkg, rec, sp, values, D, 1, graph, bodies=bodies, sources=sources, beta=BETA, ref=REF)
        for _ in range(3):
            f.DispatchN(2)
        before = (f.download(), f.scalars(), f.obstacles(), f.scalar_injected())
        f.set_obstacles(bodies[:1])                                      # source 3 rides on body 1, which is gone
        poses = f.obstacles()
        for call in (f.DispatchCompute, lambda: f.DispatchN(2)):
            with pytest.raises(pkg.SphError, match="error -3:.*obstacle 1"):
                call()
        assert_records_equal(f.download(), before[0], "a refused dispatch changes no record")
        same_bits(f.scalars(), before[1], "a refused dispatch changes no value")
        same_bits(f.obstacles(), poses, "nor a pose")
        # (a set with another obstacle count zeroes the impulse sums, not the scalar books)
        assert f.scalar_injected()[1].tolist() == before[3][1].tolist() and f.scalar_injected()[3] == 6
        f.set_scalar_sources(sources[:3])
        f.DispatchN(2)
        assert f.scalar_injected()[3] == 2
        f.close()
    # the engine-side refusals: no scalars, more than 8 sources, a bad channel; set_scalars and reset drop the coupling
    f = engine(pkg, rec, sp)
    for call in (lambda: f.set_scalar_buoyancy(1.0), lambda: f.set_scalar_sources(sources), f.scalar_injected, f.scalar_sources, f.scalar_buoyancy):
        with pytest.raises(pkg.SphError, match="error -3:"):
            call()
    f.set_scalars(values, diffusivity=D)
    f.set_scalar_sources(sources[:2])
    f.set_scalar_buoyancy(BETA, REF)
    for call in (lambda: f.set_scalar_sources(sources[:2] * 5), lambda: f.set_scalar_sources([pkg.scalar_source(0, c, 1.0, channel=K)]),
                 lambda: f.set_scalar_buoyancy((np.nan, 0.0), 0.0), lambda: f.set_scalar_sources([pkg.scalar_source(0, c, -1.0)])):
        with pytest.raises(pkg.SphError, match="error -1:"):
            call()
    assert f.scalar_sources().tobytes() == pkg.source_array(sources[:2]).tobytes()          # the previous state is kept
    same_bits(f.scalar_buoyancy()[0], BETA, "beta as set")
    same_bits(f.scalar_buoyancy()[1], REF, "ref as set")
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)                              # the linked-list variant: refused as the channels themselves are
    for call in (lambda: f.set_scalar_buoyancy(BETA, REF), lambda: f.set_scalar_sources(sources[:2])):
        with pytest.raises(pkg.SphError, match="error -3:"):
            call()
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    f.param_pause = 1
    f.DispatchCompute()
    assert f.scalar_injected()[3] == 0                                   # param_pause: nothing is counted
    f.param_pause = 0
    f.set_scalars(values, diffusivity=D)                                 # a new set starts without buoyancy and without sources
    assert len(f.scalar_sources()) == 0 and not f.scalar_buoyancy()[0].any()
    f.set_scalar_sources(sources[:2])
    f.ResetSimulation()
    with pytest.raises(pkg.SphError, match="error -3:"):
        f.scalar_sources()
    f.close()
    # a z-slab engine refuses
    import ctypes as C
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    L = pkg.load_library()
    one = np.ones(K, F)
    pf = C.POINTER(C.c_float)
    assert L.sph_scalars_set_buoyancy(slab._h, one.ctypes.data_as(pf), one.ctypes.data_as(pf)) == -3 and b"slab" in L.sph_last_error()
    assert L.sph_scalars_set_sources(slab._h, None, 0) == -3 and b"slab" in L.sph_last_error()
    slab.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_thermal_plume_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "thermal_plume", tmp_path), ["3", "8000"], timeout=120)
    assert res.returncode == 0 and "thermal_plume OK" in res.stdout
