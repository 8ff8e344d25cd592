"""Kinematic solid obstacles on the GPU (include/sph_abi.h "obstacles").

Records and poses are compared bit for bit with the oracle's substep followed by the numpy restatement tests/obstacle_ref.py.  Impulses
are exactly defined terms whose fp64 sum order is the engine's choice: the engine and the restatement (a correctly rounded sum) may differ
by at most 2 (n_terms - 1) 2^-53 sum |t_i| per component, the worst case of two sums of the same terms in different orders.
Every parity substep must touch at least 0.5 % of the fluid particles on the reference side, with at least one particle on the u_n < 0
branch, so a body that misses the fluid cannot pass."""
import re
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import obstacle_ref as R
from support import build_example, check_impulses, engine, fluid_block, run_example, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ((4096, 16), (32768, 32))
MOTIONS = ("static", "moving", "spinning")


def _body(pkg, shape, motion, rec, dt, offset=(0.0, 0.0, 0.0)):
    """One body inside the fluid block: sized from the block's extent E, moving by at most 0.04 E over 8 substeps, or turning by
    about 0.2 rad over 8 substeps."""
    c, E = fluid_block(rec)
    c = (c + F(E) * np.asarray(offset, F)).astype(F)
    if shape == R.SPHERE:
        size, rot = (0.2 * E,), (1.0, 0.0, 0.0, 0.0)
    elif shape == R.BOX:
        size, rot = (0.2 * E, 0.14 * E, 0.12 * E), (0.9, 0.2, 0.3, 0.1)
    else:
        size, rot = (0.13 * E, 0.12 * E), (0.8, -0.3, 0.1, 0.4)
    vel = (0.0, 0.0, 0.0)
    omega = (0.0, 0.0, 0.0)
    if motion == "moving":
        vel = tuple(0.04 * E / (8 * dt) * np.array([0.8, -0.5, 0.33]))
    elif motion == "spinning":
        omega = tuple(0.2 / (8 * dt) * np.array([0.3, 0.9, -0.3]))
    return pkg.obstacle(shape, c, size, rotation=rot, vel=vel, omega=omega)


def _reference(oracle, rec, sp, arr, steps, fountain=None):
    """Per substep: (records, bodies as OBSTACLE_DTYPE, impulses, info) of oracle + restatement."""
    op = to_oracle_params(oracle, sp)
    bs = R.bodies(arr, normalise=True)
    out = []
    for _ in range(steps):
        rec, bs, imp, info = R.step(oracle, rec, op, bs, fountain=fountain)
        out.append((rec, R.to_array(bs), imp, info))
    return out


def _cap(info, n_fluid, what):
    touched, neg = int(info["touched"].sum()), int(info["negative"].sum())
    assert touched >= 0.005 * n_fluid and neg >= 1, f"{what}: the reference touches {touched} of {n_fluid} fluid particles ({neg} with u_n < 0)"


@pytest.mark.parametrize("n,grid", SCENES)
def test_parity_with_oracle_and_reference(pkg, oracle, n, grid):
    rec0, sp = small_scene(pkg, n=n, grid=grid)
    n_fluid = int((rec0["isGhost"] == 0).sum())
    dt = float(sp.param_timeStep)
    for shape in (R.SPHERE, R.BOX, R.CAPSULE):
        for motion in MOTIONS:
            arr = pkg.obstacle_array([_body(pkg, shape, motion, rec0, dt)])
            ref = _reference(oracle, rec0, sp, arr, 8)
            fractions = []
            for k, (_, _, _, info) in enumerate(ref):
                _cap(info, n_fluid, f"{n}: shape {shape} {motion} substep {k}")
                fractions.append(info["touched"].sum() / n_fluid)
            print(f"{n} shape {shape} {motion}: reference touches {min(fractions):.4f}-{max(fractions):.4f} of the fluid per substep")
            for kern in (1, 2, 3):
                for aos in (0, 1):
                    what = f"{n}: shape {shape} {motion} pass {kern} aos {aos}"
                    f = engine(pkg, rec0, sp, kern, aos)
                    f.set_obstacles(arr)
                    for k, (want_rec, want_bodies, want_imp, info) in enumerate(ref):
                        f.DispatchCompute()
                        assert_records_equal(f.download(), want_rec, f"{what} substep {k}")
                        same_bits(f.obstacles(), want_bodies, f"{what} substep {k}: poses")
                        J, t, steps = f.obstacle_impulses(reset=True)
                        assert steps == 1 and t == np.float64(F(dt)), (steps, t)
                        check_impulses(J, want_imp, info, f"{what} substep {k}")
                    f.close()


def test_bodies_outside_the_container_change_nothing(pkg, oracle):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    g = pkg.compute_grid_extents(sp)
    far = np.array(list(g.gridMin), F) - F(50)
    dt = float(sp.param_timeStep)
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, far, 2.0, vel=(1.0, 0.0, 0.0)), pkg.obstacle(R.BOX, far - F(10), (1, 2, 3), omega=(0, 3, 0)),
                              pkg.obstacle(R.CAPSULE, far + F(5), (1, 2), rotation=(0.5, 0.5, 0.5, 0.5))])
    bs = R.bodies(arr)
    for aos in (0, 1):
        a, b = engine(pkg, rec0, sp, 3, aos), engine(pkg, rec0, sp, 3, aos)
        a.set_obstacles(arr)
        for k in range(8):
            a.DispatchCompute()
            b.DispatchCompute()
            assert_records_equal(a.download(), b.download(), f"aos {aos} substep {k}")
        bs_k = bs
        for _ in range(8):
            bs_k = R.advance(bs_k, dt)
        same_bits(a.obstacles(), R.to_array(bs_k), f"aos {aos}: poses")
        J, t, steps = a.obstacle_impulses()
        assert steps == 8 and (J == 0).all() and not np.signbit(J).any()
        a.close()
        b.close()


def _impulse_series(pkg, rec, sp, arr, kern, aos, steps=8):
    f = engine(pkg, rec, sp, kern, aos)
    f.set_obstacles(arr)
    out = []
    for _ in range(steps):
        f.DispatchCompute()
        out.append(f.obstacle_impulses(reset=True)[0])
    recs = f.download()
    f.close()
    return np.array(out), recs


def test_impulse_bits_do_not_depend_on_pass_aos_mode_or_run(pkg):
    rec0, sp = small_scene(pkg, n=32768, grid=32)
    dt = float(sp.param_timeStep)
    arr = pkg.obstacle_array([_body(pkg, R.SPHERE, "moving", rec0, dt, (-0.25, 0, 0)), _body(pkg, R.BOX, "spinning", rec0, dt, (0.25, 0, 0)),
                              _body(pkg, R.CAPSULE, "spinning", rec0, dt, (0, 0.2, 0.2))])
    first, recs = _impulse_series(pkg, rec0, sp, arr, 3, 1)
    assert (first != 0).any(axis=(1, 2)).all()
    for kern in (1, 2, 3):
        for aos in (0, 1):
            for run in range(2 if (kern, aos) == (3, 1) else 1):
                got, r = _impulse_series(pkg, rec0, sp, arr, kern, aos)
                same_bits(got, first, f"impulses, pass {kern} aos {aos} run {run}")
                assert_records_equal(r, recs, f"pass {kern} aos {aos}")


def test_graph_replay_sees_set_motion(pkg):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    arr = pkg.obstacle_array([_body(pkg, R.SPHERE, "moving", rec0, dt, (-0.2, 0, 0)), _body(pkg, R.BOX, "spinning", rec0, dt, (0.2, 0, 0))])
    motions = [((1.0, 0.0, 0.0), (0.0, 2.0, 0.0)), ((0.0, -2.0, 0.5), (3.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
               ((-1.5, 0.0, 1.0), (0.0, -4.0, 1.0)), ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0))]
    runs = []
    for graph in (1, 0):
        f = engine(pkg, rec0, sp, 3, 1, graph)
        f.set_obstacles(arr)
        seen = []
        for i, (v, w) in enumerate(motions):
            f.DispatchN(16)
            seen.append((f.download(), f.obstacles(), f.obstacle_impulses(reset=i % 2 == 1)))
            f.set_obstacle_motion(i % 2, v, w)
        f.DispatchN(16)
        seen.append((f.download(), f.obstacles(), f.obstacle_impulses()))
        launches = f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
        runs.append(seen)
        f.close()
        if graph:
            assert launches > 0
    for k, ((ra, oa, ja), (rb, ob, jb)) in enumerate(zip(*runs)):
        assert_records_equal(ra, rb, f"call {k}: records")
        same_bits(oa, ob, f"call {k}: poses")
        same_bits(ja[0], jb[0], f"call {k}: impulses")
        assert ja[1:] == jb[1:]
    assert (runs[0][-1][1]["vel"][0] == F(0.5)).all() and runs[0][-1][1]["omega"][1][1] == F(-4.0)   # the last set_motion of each body
    assert not np.array_equal(runs[0][1][1]["center"], runs[0][2][1]["center"])


def test_refusals_resets_pause_and_fountain(pkg, oracle):
    import ctypes as C
    L = pkg.load_library()
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    # a z-slab engine
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec0, np.arange(len(rec0), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec0) * 1.2) + 8192)
    one = pkg.obstacle_array([pkg.obstacle(R.SPHERE, (0, 0, 0), 1.0)])
    assert L.sph_obstacles_set(slab._h, one.ctypes.data_as(C.c_void_p), 1) == -3 and b"slab" in L.sph_last_error()
    slab.close()
    # SPH_ERR_ARG keeps the previous set
    a = _body(pkg, R.BOX, "moving", rec0, dt)
    b = _body(pkg, R.CAPSULE, "spinning", rec0, dt)
    f = engine(pkg, rec0, sp)
    f.set_obstacles([a, b])
    before = f.obstacles()
    bad = pkg.obstacle(R.SPHERE, (0, 0, 0), -1.0)
    for obs in ([a, bad], [bad], [a] * 17, [pkg.obstacle(7, (0, 0, 0), 1.0)], [pkg.obstacle(R.BOX, (0, 0, 0), 1.0, rotation=(0, 0, 0, 0))],
                [pkg.obstacle(R.SPHERE, (0, 0, 0), 1.0, restitution=2.0)], [pkg.obstacle(R.SPHERE, (0, float("nan"), 0), 1.0)]):
        with pytest.raises(pkg.SphError, match="-1"):
            f.set_obstacles(obs)
        same_bits(f.obstacles(), before, "a refused set keeps the previous one")
    for idx in (-1, 2):
        with pytest.raises(pkg.SphError, match="-1"):
            f.set_obstacle_motion(idx, (0, 0, 0), (0, 0, 0))
    with pytest.raises(pkg.SphError, match="-1"):
        f.set_obstacle_motion(0, (0, float("inf"), 0), (0, 0, 0))
    # the set normalises the quaternion
    assert np.array_equal(before["rotation"][0], R.normalize(np.array([0.9, 0.2, 0.3, 0.1], F)))
    # accumulators: kept by a set with the same count and by set_motion, zeroed by another count, reset=True and sph_reset
    f.DispatchN(3)
    J3, t3, n3 = f.obstacle_impulses()
    assert n3 == 3 and (J3 != 0).any()
    f.set_obstacles([a, b])
    f.set_obstacle_motion(1, (0, 0, 0), (0, 1, 0))
    f.DispatchCompute()
    J4, t4, n4 = f.obstacle_impulses(reset=True)
    assert n4 == 4 and t4 == t3 + float(F(dt))
    J0, t0, n0 = f.obstacle_impulses()
    assert J0.shape == (2, 6) and (J0 == 0).all() and (t0, n0) == (0.0, 0)
    f.DispatchCompute()
    f.set_obstacles([a])
    assert f.obstacle_impulses()[1:] == (0.0, 0) and f.obstacle_impulses()[0].shape == (1, 6)
    f.set_obstacles([a, b])
    f.DispatchN(2)
    poses = f.obstacles()
    assert f.obstacle_impulses()[2] == 2
    f.ResetSimulation()
    assert f.obstacle_impulses()[1:] == (0.0, 0)
    same_bits(f.obstacles(), poses, "sph_reset keeps the set and the current poses")
    # param_pause: nothing moves, nothing accumulates
    f.DispatchN(2)
    r, o, i = f.download(), f.obstacles(), f.obstacle_impulses()
    f.param_pause = 1
    f.DispatchCompute()
    f.DispatchN(4)
    same_bits(f.download(), r, "pause: records")
    same_bits(f.obstacles(), o, "pause: poses")
    assert f.obstacle_impulses()[1:] == i[1:] and f.obstacle_impulses()[0].tobytes() == i[0].tobytes()
    f.param_pause = 0
    f.clear_obstacles()
    assert len(f.obstacles()) == 0 and f.obstacle_impulses()[2] == 0
    f.DispatchCompute()
    f.close()
    # fountain + obstacles against the oracle in the engine's order: SPH pass, container, obstacles, fountain recycle
    e = engine(pkg, rec0, sp, 3, 0)
    e.fountainMode = 1
    e.fountainOffset = (0.0, -1.0, 0.0)
    e.fountainDrainPerSec = 200.0
    e.fountainDrainLevel = 1.5
    ff = e._f
    fo = oracle.default_fountain(mode=1, offset=list(ff.fountainOffset), radius=ff.fountainRadius, spread=ff.fountainSpread,
                                 jetSpeedLive=ff.fountainJetSpeedLive, drainLevel=ff.fountainDrainLevel, drainPerSec=ff.fountainDrainPerSec,
                                 seed=ff.fountainSeed)
    arr = pkg.obstacle_array([_body(pkg, R.SPHERE, "moving", rec0, dt, (0, -0.2, 0)), _body(pkg, R.CAPSULE, "spinning", rec0, dt, (0, 0.2, 0))])
    e.set_obstacles(arr)
    ref = _reference(oracle, rec0, sp, arr, 6, fountain=fo)
    for k, (want_rec, want_bodies, want_imp, info) in enumerate(ref):
        e.DispatchCompute()
        assert_records_equal(e.download(), want_rec, f"fountain substep {k}")
        same_bits(e.obstacles(), want_bodies, f"fountain substep {k}: poses")
        check_impulses(e.obstacle_impulses(reset=True)[0], want_imp, info, f"fountain substep {k}")
    assert e.fountainSeed == 6
    e.close()


def test_drag_opposes_the_motion_of_a_sphere(pkg):
    rec0, sp = small_scene(pkg, n=32768, grid=32)
    c, E = fluid_block(rec0)
    dt = float(sp.param_timeStep)
    V = 0.05 * E / (16 * dt)                                             # 5 % of the block over the run: the sphere stays inside the fluid
    f = engine(pkg, rec0, sp)
    f.DispatchN(4)                                                       # densities first
    f.set_obstacles([pkg.obstacle(R.SPHERE, c, 0.2 * E, vel=(V, 0.0, 0.0))])
    f.DispatchN(16)
    J, t, steps = f.obstacle_impulses()
    print(f"J = {J[0]}, t = {t}, substeps = {steps}")
    assert steps == 16 and J[0, 0] * V < 0
    f.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stirred_tank_torque_opposes_the_spin(pkg, tmp_path):
    res = run_example(build_example(pkg, "stirred_tank", tmp_path), ["10", "50000", "4.0"], timeout=300)
    assert res.returncode == 0 and "stirred_tank OK" in res.stdout
    torques = [float(x) for x in re.findall(r"torque_y=(\S+)", res.stdout)]
    assert len(torques) == 10 and all(t * 4.0 < 0 for t in torques), torques
