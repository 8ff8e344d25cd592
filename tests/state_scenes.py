"""What the checkpoint tests on the GPU share (tests/test_gpu_state.py, tests/test_gpu_fuzz_state.py): per feature a blob carries the
set-up of the run, the junk the loading engine holds of it before, and every output it has; and the comparison of two engines' outputs."""
import numpy as np

import support as T


# ---- what each feature sets up, the junk the loading engine holds of it before, and its outputs -------------------------
def _points(rec, m, seed):
    rng = np.random.default_rng(seed)
    c, ext = T.fluid_block(rec)
    return (c + (rng.random((m, 3)).astype(np.float32) - 0.5) * np.float32(0.8 * ext)).astype(np.float32)


def tracers_on(pkg, f, rec, junk=False):
    f.set_tracers(_points(rec, 40 if junk else 131, 5 + junk), integrator=pkg.SPH_TRACER_EULER if junk else pkg.SPH_TRACER_MIDPOINT,
                  history=5 if junk else 3, stride=2 if junk else 3)


def tracers_out(f):
    first, hist = f.tracer_history() if f.tracer_info()[1] else (0, np.zeros((0, f.num_tracers(), 4), np.float32))   # (a set without history has none)
    return dict(tracers=f.tracers(), tracer_info=np.array(f.tracer_info(), np.uint64), tracer_first=np.array([first], np.uint64), tracer_history=hist)


def gates_on(pkg, f, rec, junk=False):
    c, ext = T.fluid_block(rec)
    g = [pkg.gate(pkg.SPH_GATE_RECT, c, (ext, 0, 0), (0, 0, ext)), pkg.gate(pkg.SPH_GATE_ELLIPSE, c + np.float32(0.1), (0, 0.3 * ext, 0), (0, 0, 0.3 * ext))]
    f.set_gates(g[:1] if junk else g, history=7 if junk else 4, stride=1 if junk else 2)


def gates_out(f):
    rows, time, substeps = f.gate_books()
    first, hist, times = f.gate_history()
    return dict(gates=f.gates(), gate_books=rows, gate_time=np.array([time]), gate_substeps=np.array([substeps], np.uint64),
                gate_first=np.array([first], np.uint64), gate_history=hist, gate_times=times)


def monitors_on(pkg, f, rec, junk=False):
    c, ext = T.fluid_block(rec)
    if junk:
        f.set_monitor(_points(rec, 9, 77), slot=1, every=1, history=3)
        f.set_monitor(_points(rec, 30, 78), slot=3)
        return
    f.set_monitor(_points(rec, 70, 11), slot=0, every=4, history=2, stride=1, ring_points=5)
    f.set_monitor(lattice=(c - np.float32(0.3 * ext), 0.2 * ext, (5, 3, 4)), slot=2, every=4, wet_fraction=0.4, history=2, stride=1)


def monitors_out(f):
    out = {}
    for slot in range(4):
        info = f.monitor_info(slot)
        out[f"monitor_info{slot}"] = np.array([info["kind"], info["points"], info["substeps"], info["acting"], info["ringRows"], info["firstRow"]], np.int64)
        out[f"monitor_time{slot}"] = np.array([info["time"]])
        if info["kind"]:
            out[f"monitor_rows{slot}"] = f.monitor_rows(slot)
            first, samples, times = f.monitor_history(slot)
            out[f"monitor_history{slot}"] = samples
            out[f"monitor_times{slot}"] = times
    return out


def diffuse_on(pkg, f, rec, junk=False):
    c, ext = T.fluid_block(rec)
    f.set_diffuse(capacity=900 if junk else 6000, seed=17 if junk else 5, threshold=0.0, rate=40000.0, lifeMin=0.003, lifeMax=0.02, maxAge=0.05)
    pool = np.zeros(7 if junk else 60, pkg.DIFFUSE_DTYPE)                # living records from the first substep on, of every class
    pool["pos"] = _points(rec, len(pool), 31 + junk)
    pool["vel"][:, 1] = 1.0
    pool["life"] = np.linspace(0.002, 0.05, len(pool), dtype=np.float32)  # (some die within A + B substeps)
    pool["kind"] = np.arange(len(pool)) % 3
    f.seed_diffuse(pool)
    if not junk:                                                        # crest births every 4th substep: the phase must survive the load
        f.set_diffuse_crest(every=4, rate=20000.0, crestMin=-50.0, crestMax=50.0, speedMin=-1.0, speedMax=1e6, align=0.0)


def diffuse_out(f):
    info, crest = f.diffuse_info(), f.diffuse_crest_info()
    return dict(diffuse=f.diffuse(), diffuse_info=np.array([info[k] for k in sorted(info) if k != "aliveByKind"] + list(info["aliveByKind"]), np.uint64),
                diffuse_crest_info=np.array([crest[k] for k in ("acting", "crestSpawned", "shellSize", "on")], np.int64))


def scalars_on(pkg, f, rec, junk=False):
    n = len(rec)
    rng = np.random.default_rng(3 + junk)
    c, ext = T.fluid_block(rec)
    if junk:
        f.set_scalars(rng.random(n).astype(np.float32), diffusivity=0.3)
        return
    f.set_scalars(rng.random((n, 3)).astype(np.float32), diffusivity=(0.5, 0.0, 0.2), decay=(0.0, 0.1, 0.0))   # (n * 3: an odd number of words for odd n)
    f.set_scalar_buoyancy(beta=(0.02, 0.0, -0.01), ref=0.5)
    f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.3 * ext, channel=0, mode=pkg.SPH_SOURCE_RATE, rate=5.0),
                          pkg.scalar_source(pkg.SPH_SOURCE_BOX, c - np.float32(0.2 * ext), (0.2 * ext,) * 3, channel=2, mode=pkg.SPH_SOURCE_RELAX, rate=50.0, target=2.0)])


def scalars_out(f):
    sums, hits, time, substeps = f.scalar_injected()
    steps, number = f.scalar_info()
    return dict(scalars=f.scalars(), scalar_info=np.array([steps], np.uint64), scalar_number=np.array([number], np.float32), scalar_sources=f.scalar_sources(),
                scalar_injected=sums, scalar_hits=hits, scalar_time=np.array([time]), scalar_substeps=np.array([substeps], np.uint64))


def obstacles_on(pkg, f, rec, junk=False):
    c, ext = T.fluid_block(rec)
    if junk:
        f.set_obstacles([pkg.obstacle(pkg.SPH_OBSTACLE_SPHERE, c, 0.1 * ext, vel=(0.3, 0, 0))])
        f.bind_obstacle_volume(0, -1)
        f.create_volume(np.ones((3, 3, 3), np.float32), 0.1)
        return
    # a spinning paddle, a floating sphere, and a box bound to a lattice of a ball's signed distances (5 x 5 x 5: an odd number of words)
    f.set_obstacles([pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c, (0.3 * ext, 0.2 * ext, 0.05 * ext), omega=(0, 3.0, 0)),
                     pkg.obstacle(pkg.SPH_OBSTACLE_SPHERE, c + np.float32(0.25 * ext), 0.08 * ext),
                     pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c - np.float32(0.25 * ext), (0.1 * ext,) * 3, vel=(0, 0.2, 0))])
    f.set_obstacle_dynamics(1, pkg.dynamics_sphere(600.0, 0.08 * ext))
    g = (np.arange(5, dtype=np.float32) - 2.0) * np.float32(0.05 * ext)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    unused = f.create_volume(np.ones((2, 2, 2), np.float32), 0.1)        # slot 0 is given back: the ball lives in slot 1
    vid = f.create_volume((np.sqrt(x * x + y * y + z * z) - np.float32(0.08 * ext)).astype(np.float32), 0.05 * ext)
    f.destroy_volume(unused)
    f.bind_obstacle_volume(2, vid)


def obstacles_out(f):
    J, time, substeps = f.obstacle_impulses()
    k = len(f.obstacles())
    dyn = [f.obstacle_dynamics(i) for i in range(k)]
    return dict(obstacles=f.obstacles(), obstacle_impulses=J, obstacle_time=np.array([time]), obstacle_substeps=np.array([substeps], np.uint64),
                obstacle_volumes=np.array([f.obstacle_volume(i) for i in range(k)], np.int64),
                obstacle_dynamics=np.frombuffer(b"".join(bytes(d) if d is not None else b"\0" * 80 for d in dyn), np.uint8))


FEATURES = {"tracers": (tracers_on, tracers_out), "diffuse": (diffuse_on, diffuse_out), "scalars": (scalars_on, scalars_out),
            "obstacles": (obstacles_on, obstacles_out), "gates": (gates_on, gates_out), "monitors": (monitors_on, monitors_out)}


def outputs(f, names):
    out = dict(records=f.download())
    for name in names:
        out.update(FEATURES[name][1](f))
    return out


def same_outputs(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        T.same_bits(np.asarray(a[k]), np.asarray(b[k]), f"{what}: {k}")
