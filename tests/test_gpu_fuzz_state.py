"""Random call sequences with a checkpoint in the middle: one engine runs a seeded sequence of dispatches, impulses, member edits,
uploads and set / reset / clear calls of the features a blob carries (tracers, diffuse pool, scalars, obstacles, gates, monitors); at a random point its state is saved and loaded
into a second engine that began life elsewhere (another scene, other features, another pass variant, record mode and graph setting).
From then on both receive the same calls: the records, every feature output and every section digest stay equal to the end."""
import numpy as np
import pytest

from conftest import small_scene
import support as T
from state_scenes import FEATURES, _points, outputs, same_outputs

pytestmark = pytest.mark.gpu
SEEDS = [0, 1, 2, 3, 4, 5]


def draw(pkg, rng, rec):
    """One call as (name, arguments): drawn once, applied to every engine alike."""
    kind = rng.choice(["dispatch", "dispatch", "dispatch_n", "dispatch_n", "wave", "vortex", "attractor", "curl", "tracers", "gates", "monitor",
                       "monitor_lattice", "clear_monitor", "reset_books", "upload", "member", "fountain", "stencil", "diffuse", "scalars", "obstacles",
                       "clear"])
    c, ext = T.fluid_block(rec)
    if kind == "dispatch_n":
        return kind, (int(rng.integers(2, 5)),)
    if kind == "wave":
        return kind, (float(rng.uniform(0.2, 1.5)), float(rng.uniform(1, 4)), float(rng.uniform(0, 6)))
    if kind == "attractor":
        return kind, (tuple(float(x) for x in c), float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.5, 2.0)))
    if kind == "tracers":
        return kind, (_points(rec, int(rng.integers(1, 90)), int(rng.integers(1 << 30))), int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(1, 4)))
    if kind == "gates":
        g = [pkg.gate(int(rng.integers(0, 2)), c + (rng.random(3).astype(np.float32) - 0.5) * np.float32(0.4 * ext), (ext, 0, 0), (0, 0, ext))
             for _ in range(int(rng.integers(0, 4)))]
        return kind, (g, int(rng.integers(0, 4)), int(rng.integers(1, 4)))
    if kind == "monitor":
        m = int(rng.integers(1, 50))
        return kind, (_points(rec, m, int(rng.integers(1 << 30))), int(rng.integers(0, 4)), int(rng.integers(1, 5)), int(rng.integers(0, 3)), int(rng.integers(1, 3)),
                      int(rng.integers(1, m + 1)))
    if kind == "monitor_lattice":
        return kind, ((c - np.float32(0.2 * ext), 0.15 * ext, tuple(int(x) for x in rng.integers(1, 5, 3))), int(rng.integers(0, 4)), int(rng.integers(1, 5)))
    if kind == "clear_monitor":
        return kind, (int(rng.integers(0, 4)),)
    if kind == "upload":
        return kind, (int(rng.integers(1 << 30)),)
    if kind == "member":
        return kind, (str(rng.choice(["param_viscosity", "param_timeStep", "param_gravityX"])), float(rng.uniform(0.8, 1.2)))
    if kind == "stencil":
        return kind, (np.concatenate([_points(rec, 3, int(rng.integers(1 << 30))), np.ones((3, 1), np.float32)], axis=1),)
    if kind in ("diffuse", "scalars", "obstacles"):
        return kind, (rec, bool(rng.integers(0, 2)))
    if kind == "clear":
        return kind, (str(rng.choice(["diffuse", "scalars", "obstacles"])),)
    return kind, ()


def apply(pkg, f, call):
    kind, a = call
    if kind == "dispatch":
        f.DispatchCompute()
    elif kind == "dispatch_n":
        f.DispatchN(a[0])
    elif kind == "wave":
        f.ApplyWaveImpulse(a[0], a[1], a[2], (0.0, 1.0, 0.0))
    elif kind == "vortex":
        f.ApplyVortexImpulse(0.3, 0.05)
    elif kind == "attractor":
        f.ApplyAttractorImpulse(*a)
    elif kind == "curl":
        f.ApplyCurlFlow(0.2, 1.5, 0.3)
    elif kind == "tracers":
        f.set_tracers(a[0], integrator=a[1], history=a[2], stride=a[3])
    elif kind == "gates":
        f.set_gates(a[0], history=a[1], stride=a[2])
    elif kind == "monitor":
        f.set_monitor(a[0], slot=a[1], every=a[2], history=a[3], stride=a[4], ring_points=a[5] if a[3] else None)
    elif kind == "monitor_lattice":
        f.set_monitor(lattice=a[0], slot=a[1], every=a[2])
    elif kind == "clear_monitor":
        f.clear_monitor(a[0])
    elif kind == "reset_books":
        f.gate_books(reset=True)
    elif kind == "upload":
        rec = f.download()
        rng = np.random.default_rng(a[0])
        rec["vel"][:, :3] *= np.float32(0.9)
        rec["padB"][rng.integers(0, len(rec), 5)] = 0.5
        f.upload(rec)
    elif kind == "member":
        setattr(f, a[0], getattr(f, a[0]) * a[1] if a[0] != "param_gravityX" else 30.0 * (a[1] - 1.0))
    elif kind == "fountain":
        f.fountainMode = 0 if f.fountainMode else 1
        f.fountainOffset = (0.0, -1.0, 0.0)
        f.fountainRadius = 0.5
    elif kind in ("diffuse", "scalars", "obstacles"):
        FEATURES[kind][0](pkg, f, a[0], junk=a[1])
    elif kind == "clear":
        {"diffuse": lambda: f.set_diffuse(capacity=0), "scalars": f.clear_scalars, "obstacles": f.clear_obstacles}[a[0]]()
    elif kind == "stencil":
        f.SetStencilTargets(a[0])
        f.ApplyStencilAttract(0.2, 0.1)


def feature_names(f):
    return [n for n in FEATURES if n in f.state_digest()]


@pytest.mark.parametrize("seed", SEEDS)
def test_checkpoint_in_the_middle_of_a_random_sequence(pkg, seed):
    rng = np.random.default_rng(4000 + seed)
    rec, sp = small_scene(pkg, n=2000 + 97 * seed, grid=16, seed=3 + seed)
    calls = [draw(pkg, rng, rec) for _ in range(int(rng.integers(14, 22)))]
    cut = int(rng.integers(3, len(calls) - 3))
    fa = T.engine(pkg, rec, sp, kern=3, aos=1, graph=0)
    fb = T.engine(pkg, *small_scene(pkg, n=500, grid=10, seed=50 + seed), kern=2, aos=0, graph=1)
    for name in FEATURES:                                               # what the second engine holds before the load is junk
        FEATURES[name][0](pkg, fb, fb.download(), junk=True)
    fb.DispatchN(2)
    for i, call in enumerate(calls):
        print(i, call[0])
        apply(pkg, fa, call)
        if i == cut:
            fb.load_state(fa.save_state())
        if i >= cut:
            if i > cut:
                apply(pkg, fb, call)
            da, db = fa.state_digest(), fb.state_digest()
            assert da == db, f"seed {seed}: digests after call {i} ({call[0]})"
            if i in (cut, len(calls) - 1) or call[0] in ("dispatch_n", "upload"):
                names = feature_names(fa)
                same_outputs(outputs(fb, names), outputs(fa, names), f"seed {seed} after call {i} ({call[0]})")
    fa.close(); fb.close()
