"""Random call sequences around the field monitors in the style of tests/test_gpu_fuzz_gates.py: set (points or a
lattice), reset and clear on random slots, interleaved with single dispatches, DispatchN, pause toggles and sample() calls, on the scenes
of support.random_scene.

The model is the contract's bookkeeping around the host twin: per slot the counter c of non-paused substeps since the set or reset, the
acting count a, the fp64 time and the ring; before every substep the model samples the slot's points with sample() / sample_lattice() and
an acting substep feeds sph_monitor_accumulate_host.  A DispatchN the model cannot look into is run as that many single dispatches on a
second engine in lockstep, whose samples the model takes.  After every call rows, info and ring of every slot must be the model's bytes."""
import numpy as np
import pytest

import monitor_ref as MR
from support import fluid_block, random_scene

pytestmark = pytest.mark.gpu

F = np.float32
SEEDS = [3, 39, 121, 138, 223, 232, 7, 31]
CALLS = 40


class Slot:
    def __init__(self, pkg, kind, where, cfg):
        self.pkg, self.kind, self.where, self.cfg = pkg, kind, where, cfg
        self.restart()

    def restart(self):
        self.c, self.a, self.time, self.rows, self.ring = 0, 0, 0.0, None, []

    def sample(self, f):
        if self.kind == "points":
            return f.sample(self.where)
        return f.sample_lattice(*self.where, field=self.pkg.SPH_FIELD_ALL)

    def step(self, f, dt):
        """One non-paused substep is about to run on engine f (whose state the substep starts from)."""
        every, wet, history, stride, rp = self.cfg
        if MR.acts(self.c, every):
            s = self.sample(f)
            self.rows = self.pkg.monitor_accumulate_host(self.rows, s, wet)
            if MR.ring_row(self.a, history, stride) != MR.NO_ROW:
                self.ring = (self.ring + [(s.reshape(-1)[:rp].copy(), self.time)])[-history:]
            self.a += 1
        self.c += 1
        self.time = self.time + float(F(dt))

    def compare(self, f, slot, what):
        every, wet, history, stride, rp = self.cfg
        info, rows = f.monitor_info(slot), f.monitor_rows(slot)
        m = rows.size
        assert (info["substeps"], info["acting"], info["time"], info["every"], info["history"], info["stride"], info["ringPoints"]) == \
            (self.c, self.a, self.time, every, history, stride, rp), f"{what}: slot {slot}: {info} vs {(self.c, self.a, self.time, self.cfg)}"
        want = np.zeros(m, self.pkg.MONITOR_ROW_DTYPE) if self.rows is None else self.rows.reshape(-1)
        assert rows.reshape(-1).tobytes() == want.tobytes(), f"{what}: slot {slot}: rows"
        first, samples, times = f.monitor_history(slot)
        span = MR.ring_span(self.a, history, stride)
        assert (first, len(samples)) == span == (info["firstRow"], info["ringRows"]) and len(self.ring) == span[1], f"{what}: slot {slot}: ring {first} + {len(samples)} vs {span}"
        for k, (s, t) in enumerate(self.ring):
            assert samples[k].tobytes() == s.tobytes() and times[k] == t, f"{what}: slot {slot}: ring row {first + k}"


def _random_monitor(pkg, rng, c, E, sp):
    every, stride = int(rng.integers(1, 4)), int(rng.integers(1, 3))
    history = int(rng.choice([0, 2, 3]))
    if rng.random() < 0.5:
        m = int(rng.integers(1, 300))
        pts = (c + rng.uniform(-0.6, 0.6, (m, 3)) * E).astype(F)
        if m > 4 and rng.random() < 0.3:
            pts[int(rng.integers(0, m)), int(rng.integers(0, 3))] = np.nan
        kind, where, count = "points", pts, m
    else:
        dims = tuple(int(x) for x in rng.integers(1, 14, 3))
        spacing = (rng.uniform(0.2, 1.1, 3) * float(sp.param_h)).astype(F)
        origin = (c - 0.5 * spacing * (np.array(dims) - 1) + rng.uniform(-0.3, 0.3, 3) * E).astype(F)
        kind, where, count = "lattice", (origin, spacing, dims), int(np.prod(dims))
    rp = 0 if not history else (min(count, 64) if rng.random() < 0.5 else int(rng.integers(1, count + 1)))
    wet = float(F(rng.choice([0.5, 0.25, 0.9])))
    return kind, where, (every, wet, history, stride, rp)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_monitor_sequences_against_the_twin(pkg, seed):
    rec, sp, _, what = random_scene(pkg, seed)
    rng = np.random.default_rng(7000 + seed)
    c, E = fluid_block(rec) if (rec["isGhost"] == 0).any() else (np.zeros(3, F), 1.0)
    E = max(float(E), float(sp.param_h))
    aos, kern = int(rng.integers(0, 2)), int(rng.choice([1, 2, 3, 3]))
    engines = []
    for _ in range(2):                                                          # f is driven as the sequence says, g in single dispatches
        e = pkg.SPHFluidGPU.from_particles(rec, sp)
        e.set_option(pkg.SPH_OPT_AOS_MODE, aos)
        e.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, kern)
        engines.append(e)
    f, g = engines
    model, log, paused, acted = {}, [], False, 0
    ops = ["dispatch"] * 5 + ["dispatch_n"] * 3 + ["set", "set", "set", "reset", "clear", "clear_all", "pause", "sample"]
    try:
        for _ in range(CALLS):
            op = str(rng.choice(ops)) if model or rng.random() < 0.5 else "set"
            log.append(op)
            where = f"seed {seed}: {what}: after {log}"
            if op in ("dispatch", "dispatch_n"):
                n = 1 if op == "dispatch" else int(rng.integers(2, 7))
                for _ in range(n):
                    if not paused:
                        for s in model.values():
                            s.step(g, sp.param_timeStep)
                    g.DispatchCompute()
                f.DispatchN(n) if n > 1 else f.DispatchCompute()
            elif op == "set":
                slot = int(rng.integers(0, pkg.SPH_MAX_MONITORS))
                kind, pts, cfg = _random_monitor(pkg, rng, c, E, sp)
                kw = dict(slot=slot, every=cfg[0], wet_fraction=cfg[1], history=cfg[2], stride=cfg[3], ring_points=cfg[4] or None)
                f.set_monitor(pts, **kw) if kind == "points" else f.set_monitor(lattice=pts, **kw)
                model[slot] = Slot(pkg, kind, pts, cfg)
            elif op == "reset" and model:
                slot = int(rng.choice(sorted(model)))
                f.reset_monitor(slot)
                model[slot].restart()
            elif op == "clear":
                slot = int(rng.integers(0, pkg.SPH_MAX_MONITORS))
                f.clear_monitor(slot)
                model.pop(slot, None)
            elif op == "clear_all":
                f.clear_monitor()
                model.clear()
            elif op == "pause":
                paused = not paused
                f.param_pause = g.param_pause = 1 if paused else 0
            elif op == "sample":
                pts = (c + rng.uniform(-0.5, 0.5, (17, 3)) * E).astype(F)
                assert f.sample(pts).tobytes() == g.sample(pts).tobytes(), where
            for slot in range(pkg.SPH_MAX_MONITORS):
                if slot in model:
                    model[slot].compare(f, slot, where)
                else:
                    assert f.monitor_info(slot)["kind"] == pkg.SPH_MONITOR_NONE, where
            acted = max([acted] + [s.a for s in model.values()])
        assert f.download().tobytes() == g.download().tobytes(), f"seed {seed}: the monitors changed the run"
        print(f"seed {seed}: {what}: {log}: up to {acted} acting substeps on a slot")
    finally:
        f.close()
        g.close()
