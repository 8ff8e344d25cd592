"""The composed reference of tests/compose_ref.py without a GPU: before the Mirror judges a kernel it is itself checked against the
library's host twins, the generator against what it is meant to reach, and the sequences against planted wiring mistakes.

No tolerance is used here: the host twins and the mirror get the same impulse sums, so every comparison is for equal bits."""
import os

import numpy as np

from conftest import assert_records_equal, small_scene, to_oracle_params
import compose_ref as CZ
import obstacle_ref as R
import volume_ref as VR
from support import G, fluid_block, same_bits
from test_gpu_fuzz_features import SEEDS_A, SEEDS_B

F = np.float32


def _committed():
    return [("A", s) for s in SEEDS_A] + [("B", s) for s in SEEDS_B]


def test_pass_and_container_compose_to_the_substep(pkg, oracle):
    """Step 4 of the mirror's substep: oracle.sph_pass followed by oracle.obb is oracle.substep, on scenes of every container kind."""
    for seed in (0, 3, 5, 9):
        rec, sp, what, _, _ = CZ.feature_scene(pkg, seed)
        op = to_oracle_params(oracle, sp)
        for dt in (-1.0, 5e-4):
            assert_records_equal(oracle.obb(oracle.sph_pass(rec, op, dt=dt), op), oracle.substep(rec, op, dt=dt), f"{what}")


def test_one_substep_equals_the_chain_of_host_twins(pkg, oracle):
    """scene4096 after 10 substeps with two bodies (a box bound to a sphere lattice, a dynamic sphere), two channels, four sources (two of
    them riding on the bodies) and buoyancy: Mirror.substep against oracle.substep -> sph_obstacles_apply_host_volumes ->
    sph_obstacles_step_host -> sph_scalars_step_host on the entry records -> sph_scalars_couple_host, for two consecutive substeps."""
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    c, E = fluid_block(rec)
    K = 2
    values = np.random.default_rng(5).uniform(-1.0, 2.0, (len(rec), K)).astype(F)
    lat, spacing = VR.sphere_lattice(0.12 * E, 0.03 * E), 0.03 * E
    half = VR.volume(lat, spacing)["half"]
    bodies = pkg.obstacle_array([pkg.obstacle(R.BOX, c + F(0.15 * E) * np.array([1, 0, -1], F), tuple(float(x) for x in half), rotation=(0.8, 0.3, -0.4, 0.2),
                                              vel=(0.4, 0.0, -0.2), omega=(0.0, 3.0, 1.0)),
                                 pkg.obstacle(R.SPHERE, c - F(0.2 * E) * np.array([1, 1, 0], F), 0.11 * E)])
    dyn = [None, pkg.dynamics_sphere(0.6 * float(sp.param_restDensity), 0.11 * E)]
    sources = [pkg.scalar_source(pkg.SPH_SOURCE_BOX, c - F(0.3 * E) * np.array([0, 1, 0], F), (0.6 * E, 0.12 * E, 0.6 * E), channel=0, mode=pkg.SPH_SOURCE_RELAX,
                                 rate=60.0, target=2.5),
               pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.35 * E, channel=0, mode=pkg.SPH_SOURCE_RATE, rate=5.0),
               pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.04 * E, 0.0), (0.24 * E, 0.2 * E, 0.2 * E), channel=1, mode=pkg.SPH_SOURCE_RATE, rate=9.0, body=0),
               pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, (0.02 * E, 0.0, 0.0), 0.22 * E, channel=1, mode=pkg.SPH_SOURCE_RELAX, rate=2000.0, target=-0.5, body=1)]
    beta, ref = np.array([0.6, -0.3], F), np.array([0.2, 0.1], F)
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0)
    D, lam = F(0.4 / float(s1)), F(1.5)
    m = CZ.Mirror(pkg, oracle, rec, sp)
    m.set_scalars(values, D, lam)
    m.set_obstacles(bodies)
    m.create_volume("v0", lat, spacing)
    m.bind_volume(0, "v0")
    m.set_dynamics(1, dyn[1])
    m.set_sources(pkg.source_array(sources))
    m.set_buoyancy(beta, ref)
    op = to_oracle_params(oracle, sp)
    cur, cur_c, poses = rec, values, R.to_array(R.bodies(bodies, normalise=True))
    for step in range(2):
        what = f"substep {step}"
        after, J = pkg.obstacles_apply_host_volumes(poses, [(lat, spacing)], [0, -1], sp.param_mass, oracle.substep(cur, op))
        moved = pkg.obstacles_step_host(poses, dyn, J, sp, sp.param_timeStep)
        diffused, number = pkg.scalars_step_host(cur, sp, cur_c, diffusivity=D, decay=lam)
        want_rec, want_c, sums, hits = pkg.scalars_couple_host(after, sp, diffused, beta=beta, ref=ref, sources=sources, obstacles=moved)
        m.substep(impulses=J)
        assert_records_equal(m.rec, want_rec, what)
        same_bits(m.values, want_c, what + ": values")
        same_bits(m.poses(), moved, what + ": poses")
        assert m.sc_number.tobytes() == number.tobytes()
        assert (hits > 0).all() and (np.abs(J) > 0).any(axis=1).all() and (want_rec["vel"] != after["vel"]).any(), what
        inj = m.injected(reset=True)                       # (the twin sums in index order, the mirror correctly rounded: the order bound)
        assert inj[1].tolist() == hits.tolist() and inj[3] == 1 and (np.abs(inj[0] - sums) <= inj[4]).all(), what
        cur, cur_c, poses = want_rec, want_c, moved
    assert m.impulses()[2] == 2 and m.tracer_info() == (0, 0, 0)


def test_order_bound_is_the_bound_of_the_feature_tests():
    """compose_ref.order_bound over terms collected across substeps is obstacle_ref.impulse_bound and coupling_ref.books_bound of the same
    terms, to the bit: 2 (n - 1) 2^-53 sum |t|, zero for one term or none.  Two orders of the same sum lie within it."""
    import math
    import coupling_ref as CR
    t = np.random.default_rng(3).normal(0, 1, (37, 6))
    info = dict(touched=np.array([37]), abs_sum=np.abs(t).sum(axis=0)[None, :])
    assert np.array_equal(CZ.order_bound(t), R.impulse_bound(info)[0])
    assert CZ.order_bound(t[:, 0]) == CR.books_bound([37], [np.abs(t[:, 0]).sum()])[0]
    assert CZ.order_bound(t[:1]).tolist() == [0.0] * 6 and CZ.order_bound(np.zeros((0, 6))).tolist() == [0.0] * 6
    assert CZ.order_bound(t[:, 0]) == 72.0 * 2.0 ** -53 * np.abs(t[:, 0]).sum() > 0
    forward, backward = sum(t[:, 0].tolist()), sum(t[::-1, 0].tolist())
    assert max(abs(forward - math.fsum(t[:, 0])), abs(backward - math.fsum(t[:, 0]))) <= CZ.order_bound(t[:, 0])


def _graph_runs(ops):
    """Runs of >= 3 identical DispatchN calls that the engine can serve from a graph: (first index, last index, k)."""
    runs, i = [], 0
    while i < len(ops):
        op, a = ops[i]
        if op == "dispatch_n" and a["graph"]:
            j = i
            while j + 1 < len(ops) and ops[j + 1][0] == "dispatch_n" and ops[j + 1][1]["k"] == a["k"] and ops[j + 1][1]["graph"]:
                j += 1
            if j - i + 1 >= 3:
                runs.append((i, j, a["k"]))
            i = j + 1
        else:
            i += 1
    return runs


def test_the_sequences_reach_what_they_are_meant_to_reach(pkg):
    """Over the committed seeds of both families: every op at least twice, every pair of features alive together in a substep, graph
    runs, and the key-changing calls between two graph runs."""
    from collections import Counter
    from itertools import combinations
    count, pairs, runs, between = Counter(), set(), 0, Counter()
    for family, seed in _committed():
        _, _, what, ops = CZ.sequence(pkg, seed, family)
        assert what["n"] <= 4096 and min(what["dims"]) >= 5 and what["substeps"] <= 30, what
        for op, a in ops:
            count[op + (":" + a["name"] if op in ("query", "option", "param", "container") else "")] += 1
            if op in ("dispatch", "dispatch_n") and not a["paused"]:
                pairs.update(combinations(a["alive"], 2))
        rs = _graph_runs(ops)
        runs += len(rs)
        for (_, e0, k0), (s1, _, k1) in zip(rs, rs[1:]):
            if k0 != k1:
                continue
            for op, a in ops[e0 + 1:s1]:
                if op == "container": between["container"] += 1
                if op == "set_scalars": between["set_scalars"] += 1
                if op == "clear_obstacles": between["clear_obstacles"] += 1
                if op in ("bind", "unbind"): between["bind"] += 1
                if op == "sources" and a["first"]: between["first_sources"] += 1
    print(dict(count), "\npairs", len(pairs), "graph runs", runs, dict(between))
    alphabet = ["dispatch", "dispatch_n", "dispatch_refused", "wave", "vortex", "upload", "fountain", "reset", "set_scalars", "clear_scalars", "coefficients",
                "paint", "buoyancy", "sources", "injected", "set_obstacles", "clear_obstacles", "motion", "dynamics", "create_volume", "bind", "unbind",
                "destroy_volume", "destroy_refused", "impulses", "set_tracers", "clear_tracers"]
    alphabet += ["query:" + q for q in CZ.QUERIES] + ["option:" + o for o in CZ.OPTIONS]
    alphabet += ["param:param_viscosity", "param:param_gravityY", "param:param_timeStep", "param:param_pause"]
    alphabet += ["container:param_boxHalf", "container:param_boxEulerDeg", "container:param_shapeType"]
    rare = [k for k in alphabet if count[k] < 2]
    assert not rare, rare
    missing = [p for p in combinations(sorted(CZ.FEATURES), 2) if p not in pairs]
    assert not missing, missing                            # (the engine refuses none of these pairs on a single-domain engine)
    assert runs >= 3
    assert all(between[k] >= 1 for k in ("container", "set_scalars", "clear_obstacles", "bind", "first_sources")), dict(between)


# ---- planted wiring mistakes: each must change the end state of at least one committed sequence --------------------
def _order(*stages):
    assert sorted(stages) == sorted(CZ.STAGES)
    return stages


class CoupleBeforeObstacles(CZ.Mirror):
    ORDER = _order("grid", "tracers", "scalars", "sph", "couple", "obstacles", "bodies", "fountain")


class SourcesOnStalePoses(CZ.Mirror):
    def stage_couple(self, c):
        CZ.Mirror.stage_couple(self, c, bodies=c.poses_before)


class ScalarsOnExitState(CZ.Mirror):
    ORDER = _order("grid", "tracers", "sph", "scalars", "obstacles", "bodies", "couple", "fountain")

    def stage_scalars(self, c):
        CZ.Mirror.stage_scalars(self, c, rec=c.out, grid=self._grid_of(c.out))


class TracersAfterPass(CZ.Mirror):
    ORDER = _order("grid", "scalars", "sph", "tracers", "obstacles", "bodies", "couple", "fountain")

    def stage_tracers(self, c):
        CZ.Mirror.stage_tracers(self, c, rec=c.out, grid=self._grid_of(c.out))


class FountainBeforeCouple(CZ.Mirror):
    ORDER = _order("grid", "tracers", "scalars", "sph", "obstacles", "bodies", "fountain", "couple")


class ValuesBySlotAfterUpload(CZ.Mirror):
    def upload(self, rec):
        CZ.Mirror.upload(self, rec)
        if self.values is not None:
            self.values = self.values[self.o.build_grid(self.rec, self.op)["order"]]


class PausedSubstepAges(CZ.Mirror):
    def substep(self, dt=-1.0, impulses=None):
        if self.sp.param_pause and self.tr is not None:
            self.tr = self.tr.copy()
            self.tr["age"] = (self.tr["age"] + F(dt if dt > 0 else self.sp.param_timeStep)).astype(F)
        CZ.Mirror.substep(self, dt, impulses)


class ResetKeepsScalars(CZ.Mirror):
    def reset(self):
        keep = (self.values, self.D, self.lam)
        CZ.Mirror.reset(self)
        if keep[0] is not None:
            self.values, self.D, self.lam = np.resize(keep[0], (len(self.rec), keep[0].shape[1])), keep[1], keep[2]


MISTAKES = (CoupleBeforeObstacles, SourcesOnStalePoses, ScalarsOnExitState, TracersAfterPass, FountainBeforeCouple, ValuesBySlotAfterUpload,
            PausedSubstepAges, ResetKeepsScalars)


def test_every_planted_wiring_mistake_is_noticed(pkg, oracle):
    """The mirror alone, no engine: a copy with one wiring mistake must end a committed sequence in another state than the correct one.
    A mistake that goes unnoticed means tame scenes (sources that hit nothing, bodies outside the fluid): the generator has to change."""
    open_ = list(MISTAKES)
    noticed = {}
    for family, seed in _committed():
        if not open_:
            break
        rec, sp, what, ops = CZ.sequence(pkg, seed, family)
        runs = [CZ.Mirror(pkg, oracle, rec, sp)] + [cls(pkg, oracle, rec, sp) for cls in open_]
        for op, a in ops:
            for m in runs:
                CZ.apply(m, op, a)
        want = runs[0].state_bytes()
        for cls, m in zip(list(open_), runs[1:]):
            if m.state_bytes() != want:
                noticed[cls.__name__] = (family, seed)
                open_.remove(cls)
    print("noticed by (family, seed):", noticed)
    assert not open_, [cls.__name__ for cls in open_]
