"""Staging slots of the stream-ordered table uploads are reused safely (DESIGN.md "Host-side owners").

A table the kernels read from device memory is uploaded through one of four pinned slots; a slot is handed out again only after the copy
queued from it has run.  Each case queues four substeps (so the stream is busy), then six set calls with different values back to back
with nothing synchronising in between (more calls than slots), then two substeps.  Only the last call may count: every result equals,
bit for bit, that of a second engine with the same history that received the last call alone."""
import numpy as np
import pytest

from gates_ref import mixed_gates
from support import engine, fluid_block, random_scene

pytestmark = pytest.mark.gpu

F = np.float32
SCENE = 138          # the gates' and monitors' scene: 5544 particles, several blocks, fast particles
CALLS = 6


def _gates_case(pkg, rec, sp, c, E):
    tables = [mixed_gates(pkg, c + F(0.03 * i * E), 0.5 * E) for i in range(CALLS + 1)]
    return (lambda f: f.set_gates(tables[0], history=4, stride=1),
            [lambda f, t=t: f.set_gates(t, history=4, stride=1) for t in tables[1:]],
            lambda f: (f.gates().tobytes(), f.gate_books()[0].tobytes(), f.gate_history()[1].tobytes()))


def _coefficients_case(pkg, rec, sp, c, E):
    values = np.random.default_rng(5).uniform(-1.0, 2.0, (len(rec), 2)).astype(F)
    return (lambda f: f.set_scalars(values, diffusivity=0.0, decay=0.0),
            [lambda f, i=i: f.set_scalar_coefficients(diffusivity=(1e-4 * i, 0.0), decay=(0.0, 0.5 * i)) for i in range(1, CALLS + 1)],
            lambda f: (f.scalars().tobytes(),))


def _motion_case(pkg, rec, sp, c, E):
    dt = float(sp.param_timeStep)
    bodies = [pkg.obstacle(pkg.SPH_OBSTACLE_SPHERE, c - F(0.2 * E) * np.array([1, 0, 0], F), (0.15 * E,)),
              pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c + F(0.2 * E) * np.array([1, 0, 0], F), (0.15 * E, 0.1 * E, 0.1 * E))]
    speed = 0.01 * E / dt
    return (lambda f: f.set_obstacles(bodies),
            [lambda f, i=i: f.set_obstacle_motion(1, (speed * i, -speed, 0.0), (0.0, 2.0 * i, 1.0)) for i in range(1, CALLS + 1)],
            lambda f: (f.obstacles().tobytes(), f.obstacle_impulses()[0].tobytes()))


def _monitor_case(pkg, rec, sp, c, E):
    lattices = [(c - F(0.4 * E) + F(0.02 * i * E), F(0.1 * E), (9, 9, 9)) for i in range(CALLS + 1)]
    return (lambda f: f.set_monitor(lattice=lattices[0], history=2, ring_points=16),
            [lambda f, l=l: f.set_monitor(lattice=l, history=2, ring_points=16) for l in lattices[1:]],    # (a lattice set does not synchronise)
            lambda f: (f.monitor_rows().tobytes(), f.monitor_history()[1].tobytes(), repr(sorted(f.monitor_info().items()))))


CASES = {"set_gates": _gates_case, "set_scalar_coefficients": _coefficients_case, "set_obstacle_motion": _motion_case, "set_monitor": _monitor_case}


@pytest.mark.parametrize("call", sorted(CASES))
def test_more_back_to_back_uploads_than_slots(pkg, call):
    rec, sp, _, _ = random_scene(pkg, SCENE)
    c, E = fluid_block(rec)
    setup, calls, results = CASES[call](pkg, rec, sp, c, E)
    assert len(calls) == CALLS > 4                                        # (kObsSlots = 4 staging slots per table)

    def run(which):
        f = engine(pkg, rec, sp)
        try:
            setup(f)
            f.DispatchN(4)
            for one in which:
                one(f)
            f.DispatchN(2)
            return results(f) + (f.download().tobytes(),)
        finally:
            f.close()

    every, last, first = run(calls), run(calls[-1:]), run(calls[:1])
    for k, (a, b) in enumerate(zip(every, last)):
        assert a == b, f"{call}: result {k} after six calls differs from the last call alone"
    assert every[:-1] != first[:-1], f"{call}: the first and the last call must not give the same result (the case would show nothing)"
