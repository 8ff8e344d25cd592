"""Random call sequences around the flow gates in the style of tests/test_gpu_fuzz_features.py: set, clear,
dispatch, read with and without reset, history reads and set_params, interleaved with scalars (values, sources, buoyancy) and obstacles,
on the scenes of support.random_scene.

The model is the contract's bookkeeping around the host twin: the records (and values) are downloaded around every single dispatch and
fed to sph_gates_step_host; a set call with another count, history or stride zeroes books and ring, one with the same three keeps them;
a read with reset zeroes the books, not the ring; every `stride` substeps since the ring was zeroed the cumulative books go into a ring
row.  After every call the engine's books, time, substeps and ring must be the model's: counts exactly, the fp64 sums within
coupling_ref.books_bound of the restatement's correctly rounded sums over all terms since the last zeroing."""
import numpy as np
import pytest

import gates_ref as GR
from support import fluid_block, random_scene

pytestmark = pytest.mark.gpu

F = np.float32
SEEDS = [3, 39, 121, 138, 223, 232, 7, 31, 64, 90]
CALLS = 28


def _random_gates(pkg, rng, c, E):
    out = []
    for _ in range(int(rng.integers(1, pkg.SPH_MAX_GATES + 1))):
        q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        u, v = q[:, 0] * rng.uniform(0.05, 0.6) * E, q[:, 1] * rng.uniform(0.05, 0.6) * E
        out.append(pkg.gate(int(rng.integers(0, 2)), c + rng.uniform(-0.3, 0.3, 3) * E, u, v, unbounded=bool(rng.random() < 0.3)))
    return out


class Model:
    """What the contract says the engine holds, fed by the twin."""

    def __init__(self, pkg):
        self.pkg, self.gates, self.H, self.S = pkg, [], 0, 1
        self.zero(ring=True)

    def zero(self, ring):
        self.twin = np.zeros(len(self.gates), self.pkg.GATE_BOOKS_DTYPE)
        self.total, self.time, self.steps = None, 0.0, 0
        if ring:
            self.ring_steps, self.rows = 0, []

    def set(self, gates, H, S):
        if (len(gates), H, S) != (len(self.gates), self.H, self.S):
            self.gates, self.H, self.S = list(gates), H, S
            self.zero(ring=True)
        self.gates = list(gates)

    def step(self, before, after, values, dt):
        if not self.gates:
            return
        ref = self.pkg.gate_array(self.gates).view(GR.GATE_DTYPE)
        self.twin = self.pkg.gates_step_host(before, after, self.gates, values, self.twin)
        self.total = GR.add(self.total, GR.step(before, after, ref, values))
        self.time += float(F(dt))
        self.steps += 1
        self.ring_steps += 1
        if self.H and self.ring_steps % self.S == 0:
            self.rows.append((self.twin.copy(), {k: v.copy() for k, v in self.total.items()}, self.time))
            self.rows = self.rows[-self.H:]

    def check(self, rows, total, what):
        if total is None:
            assert not rows["forward"].any() and not rows["backward"].any() and not rows["vel"].any() and not rows["scalar"].any(), what
        else:
            GR.check_books({k: rows[k] for k in ("forward", "backward", "vel", "scalar")}, total, what)

    def compare(self, f, what, got=None):
        rows, t, n = f.gate_books() if got is None else got
        assert len(rows) == len(self.gates) and (t, n) == (self.time, self.steps), f"{what}: {(len(rows), t, n)} vs {(len(self.gates), self.time, self.steps)}"
        if self.gates:
            assert rows["forward"].tolist() == self.twin["forward"].tolist() and rows["backward"].tolist() == self.twin["backward"].tolist(), what
        self.check(rows, self.total, what)
        first, hist, times = f.gate_history()
        taken = self.ring_steps // self.S if (self.H and self.gates) else 0
        assert len(hist) == len(self.rows if self.gates else []) and first == taken - len(hist), f"{what}: ring {first} + {len(hist)} of {taken}"
        for k, (twin, total, tm) in enumerate(self.rows if self.gates else []):
            assert hist[k]["forward"].tolist() == twin["forward"].tolist() and times[k] == tm, f"{what}: ring row {k}"
            self.check(hist[k], total, f"{what}: ring row {k}")


@pytest.mark.parametrize("seed", SEEDS)
def test_random_gate_sequences_against_the_twin(pkg, seed):
    rec, sp, _, what = random_scene(pkg, seed)
    rng = np.random.default_rng(5000 + seed)
    c, E = fluid_block(rec) if (rec["isGhost"] == 0).any() else (np.zeros(3, F), 1.0)
    E = max(float(E), float(sp.param_h))
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_AOS_MODE, int(rng.integers(0, 2)))
    f.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, int(rng.choice([1, 2, 3, 3])))
    m = Model(pkg)
    log, crossings = [], 0
    ops = ["dispatch"] * 8 + ["set", "set", "same", "clear", "books", "reset", "params", "scalars", "sources", "buoyancy", "obstacles"]
    try:
        before = f.download()
        f.set_gates(g := _random_gates(pkg, rng, c, E), history=3, stride=2)
        m.set(g, 3, 2)
        for _ in range(CALLS):
            op = str(rng.choice(ops))
            log.append(op)
            where = f"seed {seed}: {what}: after {log}"
            K = f.num_scalar_channels()
            if op == "dispatch":
                dt = float(rng.choice([-1.0, -1.0, 0.5 * sp.param_timeStep]))
                f.DispatchCompute(dt)
                after = f.download()
                m.step(before, after, f.scalars() if K else None, dt if dt > 0 else f.param_timeStep)
                before = after
            elif op in ("set", "same"):
                g = _random_gates(pkg, rng, c, E)
                H, S = (m.H, m.S) if op == "same" else (int(rng.choice([0, 2, 5])), int(rng.integers(1, 4)))
                if op == "same" and m.gates:
                    g = (g * pkg.SPH_MAX_GATES)[:len(m.gates)]
                f.set_gates(g, history=H, stride=S)
                m.set(g, H, S)
            elif op == "clear":
                f.clear_gates()
                m.set([], 0, 1)
            elif op in ("books", "reset"):
                got = f.gate_books(reset=op == "reset")
                m.compare(f, where, got)
                if op == "reset":
                    m.zero(ring=False)
            elif op == "params":
                f.param_viscosity = float(rng.uniform(1.0, 6.0))
                f.param_gravityX = float(rng.uniform(-200.0, 200.0))
            elif op == "scalars":
                k = int(rng.integers(0, 5))
                if k:
                    f.set_scalars(rng.uniform(-1.0, 2.0, (len(rec), k)).astype(F), diffusivity=0.0)
                else:
                    f.clear_scalars()
            elif op == "sources" and K:
                f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.4 * E, channel=int(rng.integers(0, K)), rate=float(rng.uniform(1, 50)))])
            elif op == "buoyancy" and K:
                f.set_scalar_buoyancy(rng.uniform(-0.5, 0.5, K).astype(F), np.zeros(K, F))
            elif op == "obstacles":
                f.set_obstacles([] if rng.random() < 0.3 else [pkg.obstacle(0, c + rng.uniform(-0.2, 0.2, 3) * E, 0.2 * E, vel=tuple(rng.uniform(-1, 1, 3)))])
            m.compare(f, where)
            if m.total is not None:
                crossings = max(crossings, int((m.total["forward"] + m.total["backward"]).sum()))
        print(f"seed {seed}: {what}: {log}: up to {crossings} crossings on the books")
    finally:
        f.close()
