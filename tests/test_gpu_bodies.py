"""Dynamic rigid bodies on the GPU (include/sph_abi.h "dynamic rigid bodies").

The device is checked one step ahead: before each substep its own state is downloaded, after it the records must equal oracle +
restatement from that state bit for bit, the sums must lie within the order bound of a correctly rounded sum, and the new poses and
velocities must equal tests/body_ref.py fed with the device's own sums, bit for bit.  Long trajectories are not compared bit for bit: a
last-bit difference in a sum legitimately changes them; they are compared by what they mean (test_floating_on_the_device).  The bounds are
those of tests/test_bodies_cpu.py, where they are derived."""
import os
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import body_ref as B
import body_scenes as S
import obstacle_ref as R
import volume_ref as VR
from support import build_example, engine, fluid_block, run_example, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _scene4096(pkg):
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    return (rec, sp, *fluid_block(rec))


def _four_bodies(pkg, sp, c, E, confined=True):
    """A dynamic sphere, a dynamic box bound to a sphere lattice, a dynamic capsule with an off-centre mass and a kinematic box."""
    Rs = 0.14 * E
    sph = (VR.sphere_lattice(Rs, Rs / 5.0), Rs / 5.0)
    half = VR.volume(*sph)["half"]
    off = lambda x, y, z: (c + F(E) * np.array([x, y, z], F)).astype(F)
    dt = float(sp.param_timeStep)
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, off(-0.25, 0.1, -0.2), 0.12 * E, omega=(1.0, 0.0, 2.0)),
                              pkg.obstacle(R.BOX, off(0.25, 0.0, 0.2), half, rotation=(0.9, 0.2, 0.3, 0.1)),
                              pkg.obstacle(R.CAPSULE, off(-0.2, -0.1, 0.25), (0.08 * E, 0.1 * E), rotation=(0.8, -0.3, 0.1, 0.4)),
                              pkg.obstacle(R.BOX, off(0.2, 0.1, -0.25), (0.1 * E, 0.07 * E, 0.08 * E), vel=tuple(0.03 * E / (30 * dt) * np.array([0.5, -0.8, 0.3])),
                                           omega=(0.0, 3.0, 1.0))])
    rho = float(sp.param_restDensity)
    a = np.array([[1.0, 0.1, 0.0], [0.1, 0.8, -0.1], [0.0, -0.1, 0.6]]) * (0.8 * rho * (0.1 * E) ** 5)
    dyn = [pkg.dynamics_sphere(0.5 * rho, 0.12 * E, confined=confined), pkg.dynamics_sphere(0.8 * rho, Rs, confined=confined, angular_damping=2.0),
           pkg.dynamics(2.0 * rho * 4.0 * (0.08 * E) ** 2 * 0.2 * E, a * 30.0, com=(0.0, -0.03 * E, 0.01 * E), linear_damping=0.5, torque=(0.0, 0.0, 1e-3), confined=confined),
           None]
    return arr, dyn, [sph], [-1, 0, -1, -1]


def _set_all(f, arr, dyn, vols, bindings):
    f.set_obstacles(arr)
    ids = [f.create_volume(v, h) for v, h in vols]
    for i, b in enumerate(bindings):
        if b >= 0:
            f.bind_obstacle_volume(i, ids[b])
    for i, d in enumerate(dyn):
        if d is not None:
            f.set_obstacle_dynamics(i, d)
    return ids


def test_one_step_ahead(pkg, oracle):
    rec0, sp, c, E = _scene4096(pkg)
    op = to_oracle_params(oracle, sp)
    W = S.world_of(pkg, sp)
    dt = F(sp.param_timeStep)
    arr, dyn, vols, bindings = _four_bodies(pkg, sp, c, E)
    ds = [B.record(x) for x in pkg.dynamics_array(dyn)]
    rv = [VR.volume(v, h) for v, h in vols]
    n_fluid = int((rec0["isGhost"] == 0).sum())
    for kern, aos in ((3, 1), (2, 0)):
        f = engine(pkg, rec0, sp, kern, aos)
        _set_all(f, arr, dyn, vols, bindings)
        for i, d in enumerate(dyn):
            got = f.obstacle_dynamics(i)
            assert (got is None) == (d is None) and (d is None or bytes(got) == bytes(d))
        touched = 0
        for k in range(30):
            what = f"pass {kern} aos {aos} substep {k}"
            rec, bodies = f.download(), f.obstacles()
            f.DispatchCompute()
            J, t, steps = f.obstacle_impulses(reset=True)
            assert steps == 1 and t == np.float64(dt)
            bs = R.bodies(bodies, normalise=False)
            want_rec, want_imp, info = VR.apply(bs, rv, bindings, F(op.mass), oracle.substep(rec, op, dt=-1.0))
            assert_records_equal(f.download(), want_rec, what)
            bound = R.impulse_bound(info)
            assert (np.abs(J - want_imp) <= bound).all(), f"{what}: |engine - reference| {np.abs(J - want_imp)} above {bound}"
            same_bits(f.obstacles(), R.to_array(B.step_all(bs, ds, J, W, dt)), f"{what}: poses and velocities")
            touched += int(info["touched"].sum())
        print(f"pass {kern} aos {aos}: the reference touches {touched / 30:.1f} of {n_fluid} fluid particles per substep")
        assert touched >= 30 * 0.005 * n_fluid
        f.close()


def test_replay_equals_single_dispatches(pkg):
    rec0, sp, c, E = _scene4096(pkg)
    arr, dyn, vols, bindings = _four_bodies(pkg, sp, c, E)
    rho = float(sp.param_restDensity)
    runs = []
    for mode in ("graph", "dispatch_n", "single"):
        f = engine(pkg, rec0, sp, 3, 1, 1 if mode == "graph" else 0)
        _set_all(f, arr, dyn, vols, bindings)
        seen = []
        for call in range(4):
            if mode == "single":
                for _ in range(64):
                    f.DispatchCompute()
            else:
                f.DispatchN(64)
            seen.append((f.download(), f.obstacles(), f.obstacle_impulses()))
            if call == 0:
                f.set_obstacle_dynamics(0, pkg.dynamics_sphere(3.0 * rho, 0.12 * E))   # the floater becomes a sinker
            if call == 1:
                f.set_obstacle_motion(2, (0.0, 5.0, 0.0), (0.0, 0.0, 8.0))         # a kick
                kicked = f.obstacles()
                assert kicked["vel"][2].tolist() == [0.0, 5.0, 0.0] and kicked["omega"][2].tolist() == [0.0, 0.0, 8.0]
            if call == 2:
                f.set_obstacle_dynamics(1, None)                                   # kinematic again, at the velocity it has
        launches = f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
        runs.append(seen)
        f.close()
        if mode == "graph":
            assert launches > 0
    for other, name in ((runs[0], "graph"), (runs[1], "dispatch_n")):
        for k, ((ra, oa, ja), (rb, ob, jb)) in enumerate(zip(other, runs[2])):
            assert_records_equal(ra, rb, f"{name}, call {k}: records")
            same_bits(oa, ob, f"{name}, call {k}: poses")
            same_bits(ja[0], jb[0], f"{name}, call {k}: accumulators")
            assert ja[1:] == jb[1:]
    # the changes took effect: another mass sinks, the kick is visible, the kinematic body keeps its velocity
    plain = engine(pkg, rec0, sp, 3, 1, 0)
    _set_all(plain, arr, dyn, vols, bindings)
    plain.DispatchN(128)
    assert not np.array_equal(plain.obstacles()["center"][0], runs[2][1][1]["center"][0])
    plain.close()
    same_bits(runs[2][3][1]["vel"][1], runs[2][2][1]["vel"][1], "a body made kinematic keeps its velocity")
    assert all(np.isfinite(o[f]).all() for _, o, _ in runs[2] for f in ("center", "rotation", "vel", "omega"))


def test_momentum_ledger_on_the_device(pkg):
    """The ledger of tests/test_bodies_cpu.py::test_momentum_ledger (derived there) over 200 substeps, the sums read from the accumulators."""
    rec0, sp, c, E = _scene4096(pkg)
    arr, dyn, vols, bindings = _four_bodies(pkg, sp, c, E, confined=False)
    rho = float(sp.param_restDensity)
    dyn[1] = pkg.dynamics_sphere(0.8 * rho, 0.14 * E, confined=False)
    dyn[2] = pkg.dynamics_capsule(2.0 * rho, (0.08 * E, 0.1 * E), confined=False)
    f = engine(pkg, rec0, sp)
    _set_all(f, arr, dyn, vols, bindings)
    dt = F(sp.param_timeStep)
    push = np.array([float(F(dt * F(x))) for x in (sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ)])
    mass = np.array([float(d.mass) for d in dyn[:3]])
    cur = f.obstacles()
    worst, pushed = 0.0, 0
    for k in range(200):
        f.DispatchCompute()
        J = f.obstacle_impulses(reset=True)[0][:3, :3]
        new = f.obstacles()
        V, V1 = cur["vel"][:3].astype(np.float64), new["vel"][:3].astype(np.float64)
        jm32 = (J / mass[:, None]).astype(F)
        t1 = (cur["vel"][:3] + jm32).astype(F)
        X = np.maximum(np.maximum(np.abs(jm32), np.abs(t1)), np.abs(new["vel"][:3]))
        bound = mass[:, None] * (1.5 * np.spacing(X).astype(np.float64) + 2.0 ** -52 * np.abs(J / mass[:, None]))
        res = np.abs(mass[:, None] * (V1 - V) - J - mass[:, None] * push[None, :])
        assert (res <= bound).all(), f"substep {k}: residual {res} above {bound}"
        worst = max(worst, float((res / bound).max()))
        pushed += int((J != 0).any(axis=1).sum())
        same_bits(new["vel"][3], cur["vel"][3], "the kinematic body keeps its velocity")
        cur = new
    print(f"largest residual / bound over 200 substeps: {worst:.3g}; body-substeps with a fluid impulse: {pushed} of 600")
    assert pushed >= 100
    f.close()


def test_floating_on_the_device(pkg, oracle):
    """The floating scene of tests/test_bodies_cpu.py::test_floating on the device, with the same assertions (derived there)."""
    rec0, sp, arr, dyn = S.floating_scene(pkg)
    dt = F(sp.param_timeStep)
    f = engine(pkg, rec0, sp)
    f.set_obstacles(arr)
    for i, d in enumerate(dyn):
        f.set_obstacle_dynamics(i, d)
    H, JY, excess = [], [], -1.0
    bs = R.bodies(f.obstacles(), normalise=False)
    for _ in range(S.FLOAT_STEPS):
        f.DispatchCompute()
        J = f.obstacle_impulses(reset=True)[0]
        cur = f.obstacles()
        assert np.isfinite(J).all() and all(np.isfinite(cur[x]).all() for x in ("center", "rotation", "vel", "omega")), "a record is not finite"
        before, bs = bs, R.bodies(cur, normalise=False)
        rec = f.download()
        p = rec["pos"][rec["isGhost"] == 0][:, :3]
        for b0, b1 in zip(before, bs):
            excess = max(excess, float(S.depth(b1, p).max()) - S.depth_allowance(b0, b1, p, dt))
        H.append(cur["center"][:, 1].astype(np.float64))
        JY.append(J[:, 1].copy())
    f.close()
    # the restatement's own run
    op = to_oracle_params(oracle, sp)
    W = S.world_of(pkg, sp)
    ds = [B.record(x) for x in pkg.dynamics_array(dyn)]
    rb = R.bodies(arr, normalise=True)
    rec, rH, rJY = rec0, [], []
    for _ in range(S.FLOAT_STEPS):
        rec, imp, _ = R.apply(rb, F(sp.param_mass), oracle.substep(rec, op, dt=-1.0))
        rb = B.step_all(rb, ds, imp, W, dt)
        rH.append([float(b["c"][1]) for b in rb])
        rJY.append(imp[:, 1].copy())
    wdt = np.array([float(d.mass) for d in dyn]) * abs(float(sp.param_gravityY)) * float(dt)
    floor = float(sp.param_boxCenter[1]) - float(pkg.effective_half(sp)[1])
    h, ratio, _ = S.floating_measures(H, JY, wdt)
    rh, rratio, rwin = S.floating_measures(rH, rJY, wdt)
    S.check_floating(h, ratio, rh, rratio, rwin, floor, "device")
    rest = floor + S.FLOAT_R
    print(f"heavy sphere: mean height {h[2]!r}, floor + R = {rest}; worst depth minus allowance {excess:.3g}")
    assert abs(h[2] - rest) <= np.spacing(F(abs(rest)))
    assert excess <= 0.0


def test_kinematic_behaviour_is_unchanged(pkg):
    rec0, sp, c, E = _scene4096(pkg)
    arr, dyn, vols, bindings = _four_bodies(pkg, sp, c, E)
    arr["vel"][0] = (0.5, -0.2, 0.1)
    out = []
    for with_dynamics in (True, False):
        f = engine(pkg, rec0, sp, 3, 1, 1)
        f.set_obstacles(arr)
        if with_dynamics:
            for i in (0, 2):
                f.set_obstacle_dynamics(i, dyn[i])
            for i in (0, 2):
                f.set_obstacle_dynamics(i, None)
        f.DispatchN(8)
        f.DispatchCompute()
        out.append((f.download(), f.obstacles(), f.obstacle_impulses()))
        f.close()
    assert_records_equal(out[0][0], out[1][0], "records")
    same_bits(out[0][1], out[1][1], "poses")
    same_bits(out[0][2][0], out[1][2][0], "accumulators")
    assert out[0][2][1:] == out[1][2][1:]


def test_moments_on_the_device(pkg):
    """Against the host twin within the order bound 2 (n - 1) 2^-53 sum |t| cell, on lattices that split differently over the kernel's fixed
    grid: one below a single sweep of a block, one of a few blocks, one larger than the whole grid's first sweep (the grid-stride loop)."""
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    f = engine(pkg, rec0, sp)
    for name, values, h in (("9^3", VR.sphere_lattice(0.1, 0.1, margin=3), 0.1), ("41^3", VR.sphere_lattice(0.85, 0.05), 0.05),
                            ("box 61 x 41 x 51", VR.box_lattice((0.5, 0.3, 0.4), 0.02, margin=5), 0.02), ("141^3", VR.sphere_lattice(0.67, 0.01), 0.01)):
        vid = f.create_volume(values, h)
        got = f.volume_moments(vid)
        again = f.volume_moments(vid)
        host = pkg.volume_moments_host(values, h)
        want, bound = B.moments(values, h)
        print(f"{name}: {values.size} points, volume {got[0]:.6g}; max |device - host| / bound = {(np.abs(got - host) / np.maximum(bound, 1e-300)).max():.3g}")
        same_bits(got, again, f"{name}: two runs")
        assert (np.abs(got - host) <= bound).all() and (np.abs(got - want) <= bound).all(), f"{name}: {np.abs(got - host)} above {bound}"
        assert got[0] > 0
        mass, com, inertia = f.volume_mass_properties(vid, 2.0)
        assert mass == 2.0 * got[0] and np.abs(com).max() < 1e-5
        f.destroy_volume(vid)
    assert values.size > 2048 * 1024                                      # the last lattice is larger than one sweep of the whole grid
    with pytest.raises(pkg.SphError, match="-1"):
        f.volume_moments(3)
    f.close()


def test_refusals_and_state_changes(pkg):
    import ctypes as C
    L = pkg.load_library()
    rec0, sp, c, E = _scene4096(pkg)
    arr, dyn, vols, bindings = _four_bodies(pkg, sp, c, E)
    # a z-slab engine
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec0, np.arange(len(rec0), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec0) * 1.2) + 8192)
    assert L.sph_obstacles_set_dynamics(slab._h, 0, C.byref(dyn[0])) == -3 and b"slab" in L.sph_last_error()
    slab.close()
    f = engine(pkg, rec0, sp)
    _set_all(f, arr, dyn, vols, bindings)
    good = dyn[0]

    def bad(**kw):
        d = pkg.SphObstacleDynamics.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            cur = getattr(d, k)
            if hasattr(cur, "__len__"):
                cur[:] = v
            else:
                setattr(d, k, v)
        return d
    f.DispatchN(2)
    ref = engine(pkg, rec0, sp)
    _set_all(ref, arr, dyn, vols, bindings)
    ref.DispatchN(2)
    for what, (idx, d) in {"mass 0": (0, bad(mass=0.0)), "negative mass": (0, bad(mass=-2.0)), "nan field": (0, bad(gravityScale=float("nan"))),
                           "inf torque": (2, bad(torque=(float("inf"), 0.0, 0.0))), "negative damping": (0, bad(angularDamping=-0.5)),
                           "indefinite inertia": (0, bad(inertia=(1.0, 1.0, 1.0, 0.9, 0.9, -0.9))), "zero inertia": (0, bad(inertia=(0.0,) * 6)),
                           "index -1": (-1, good), "index 4": (4, good)}.items():
        with pytest.raises(pkg.SphError, match="-1"):
            f.set_obstacle_dynamics(idx, d)
    with pytest.raises(pkg.SphError, match="-1"):
        f.obstacle_dynamics(4)
    for i, d in enumerate(dyn):
        got = f.obstacle_dynamics(i)
        assert (got is None) == (d is None) and (d is None or bytes(got) == bytes(d)), f"a refused record replaced that of body {i}"
    f.DispatchN(3)
    ref.DispatchN(3)
    same_bits(f.obstacles(), ref.obstacles(), "refused records change nothing on the device")
    # sph_reset keeps the records, param_pause moves nothing, a set clears the records
    f.ResetSimulation()
    assert f.obstacle_dynamics(0) is not None
    before = f.obstacles()
    f.DispatchCompute()
    after = f.obstacles()
    assert not np.array_equal(before["vel"][0], after["vel"][0])          # still dynamic: gravity acts
    f.param_pause = 1
    f.DispatchN(4)
    same_bits(f.obstacles(), after, "pause")
    f.param_pause = 0
    f.set_obstacles(after)
    assert all(f.obstacle_dynamics(i) is None for i in range(4))
    f.DispatchCompute()
    same_bits(f.obstacles()["vel"], after["vel"], "a set clears the dynamics: every body is kinematic")
    f.close()
    ref.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_floating_bodies_example(pkg, tmp_path):
    res = run_example(build_example(pkg, "floating_bodies", tmp_path), ["20", "50000"], timeout=600)
    assert res.returncode == 0 and "floating_bodies OK" in res.stdout
