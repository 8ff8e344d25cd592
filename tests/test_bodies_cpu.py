"""Dynamic rigid bodies without a GPU: the host entry points (sph_obstacles_step_host, sph_volume_moments_host: the
same __host__ __device__ functions the kernels run) against the numpy restatement tests/body_ref.py, the C layout of SphObstacleDynamics,
known answers, the momentum ledger, the floating scene, the moments of lattice bodies, and the refusals.

Bounds used below and where they come from:
* Host step: every operation of section 3g is defined, so the comparison is bit for bit.
* Momentum ledger: see test_momentum_ledger.
* Floating scene: see test_floating.
* Moments: the terms are exactly defined, only the order of their fp64 sum is free; two sums of the same n terms in different orders
  differ by at most 2 (n - 1) 2^-53 sum |t_i| (tests/test_obstacles_cpu.py).  The volume bound follows from the weight rule: see
  test_moments_of_mesh_lattices.
"""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, small_scene, to_oracle_params
import body_ref as B
import body_scenes as S
import obstacle_ref as R
import volume_ref as VR
from support import build_example, c_layout, check_shim_syntax, same_bits

F = np.float32
U = 2.0 ** -24
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BODY_SYMBOLS = ("sph_obstacle_dynamics_default", "sph_obstacles_set_dynamics", "sph_obstacles_get_dynamics", "sph_obstacles_step_host",
                "sph_volume_moments", "sph_volume_moments_host")


def _rotated_params(pkg, **kw):
    return pkg.default_params(param_boxHalf=(3.0, 2.0, 2.5), param_boxEulerDeg=(10.0, -25.0, 40.0), param_boxCenter=(0.2, -0.1, 0.3), **kw)


# ---- 1. exports and layout --------------------------------------------------------------------------
def test_library_exports_the_dynamics_interface(pkg):
    L = pkg.load_library()
    for name in BODY_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphObstacleDynamics) == 80 and pkg.DYNAMICS_DTYPE.itemsize == 80 and B.DYNAMICS_DTYPE == pkg.DYNAMICS_DTYPE
    assert C.sizeof(pkg.SphObstacle) == 76                                 # SphObstacle stays what it is
    eng = open(os.path.join(ROOT, PKG_NAME, "csrc", "sph_engine.hip")).read()
    assert "static_assert(sizeof(SphObstacleDynamics) == 80" in eng
    for m in ("set_obstacle_dynamics", "obstacle_dynamics", "volume_moments", "volume_mass_properties"):
        assert hasattr(pkg.SPHFluidGPU, m), m
    d = pkg.SphObstacleDynamics()
    L.sph_obstacle_dynamics_default(C.byref(d))
    assert (d.mass, list(d.inertia), list(d.com), d.gravityScale, d.linearDamping, d.angularDamping, d.flags) == \
        (1.0, [1.0, 1.0, 1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1.0, 0.0, 0.0, pkg.SPH_DYNAMICS_CONFINED)
    # the closed forms
    s = pkg.dynamics_sphere(2.0, 0.5)
    m = 2.0 * 4.0 / 3.0 * math.pi * 0.125
    assert s.mass == F(m) and list(s.inertia) == [F(0.4 * m * 0.25)] * 3 + [0.0] * 3
    b = pkg.dynamics_box(3.0, (0.8, 0.3, 0.5))
    m = 3.0 * 8 * 0.8 * 0.3 * 0.5
    assert b.mass == F(m) and list(b.inertia)[:3] == [F(m * (0.09 + 0.25) / 3), F(m * (0.64 + 0.25) / 3), F(m * (0.64 + 0.09) / 3)]
    # the capsule against a quadrature of the same solid (midpoint rule over discs along the axis)
    r, Lh = 0.3, 0.4
    c = pkg.dynamics_capsule(1.5, (r, Lh))
    y = (np.arange(200000) + 0.5) / 200000 * 2 * (Lh + r) - (Lh + r)
    rad2 = np.where(np.abs(y) <= Lh, r * r, r * r - (np.abs(y) - Lh) ** 2)
    dy = 2 * (Lh + r) / 200000
    mass = 1.5 * math.pi * (rad2 * dy).sum()
    iy = 1.5 * math.pi * (0.5 * rad2 * rad2 * dy).sum()
    it = 1.5 * math.pi * ((0.25 * rad2 * rad2 + rad2 * y * y) * dy).sum()
    assert abs(c.mass - mass) < 1e-6 * mass and abs(c.inertia[1] - iy) < 1e-6 * iy and abs(c.inertia[0] - it) < 1e-6 * it and c.inertia[0] == c.inertia[2]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_dynamics_mirror_matches_the_header(pkg, tmp_path):
    """sizeof and every offsetof of SphObstacleDynamics (and sizeof SphObstacle), printed by C99 compiled against the header."""
    size, offsets, extra = c_layout("SphObstacleDynamics", pkg.SphObstacleDynamics, [
        'printf("SphObstacle %zu\\n", sizeof(SphObstacle));', 'printf("flag %u\\n", SPH_DYNAMICS_CONFINED);'], tmp_path)
    assert size == 80
    assert len(offsets) == len(pkg.SphObstacleDynamics._fields_)
    for (name, val), (fname, _) in zip(offsets, pkg.SphObstacleDynamics._fields_):
        assert name == fname and val == getattr(pkg.SphObstacleDynamics, fname).offset == pkg.DYNAMICS_DTYPE.fields[fname][1], (name, val)
    assert extra == ["SphObstacle 76", f"flag {pkg.SPH_DYNAMICS_CONFINED}"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_floating_bodies_compiles_and_links_against_the_c_abi(pkg, tmp_path):
    check_shim_syntax()
    assert os.path.exists(build_example(pkg, "floating_bodies", tmp_path, werror=True))


# ---- 2. the host step against the restatement -------------------------------------------------------
def _random_case(pkg, rng, sp, A, half, i):
    """One body somewhere in the rotated container, near k = 0..3 of its faces, with a random dynamics record and random sums."""
    shape = i % 3
    size = {R.SPHERE: (0.5,), R.BOX: (0.5, 0.3, 0.4), R.CAPSULE: (0.3, 0.4)}[shape]
    k = i % 4
    loc = rng.uniform(-0.5, 0.5, 3) * half
    for a in rng.permutation(3)[:k]:
        loc[a] = rng.choice([-1.0, 1.0]) * (half[a] - rng.uniform(0.0, 0.25))
    c = np.array(list(sp.param_boxCenter)) + A.reshape(3, 3).T.astype(np.float64) @ loc
    o = pkg.obstacle(shape, c, size, rotation=R.normalize(rng.standard_normal(4).astype(F)), vel=rng.standard_normal(3) * 3, omega=rng.standard_normal(3) * 2)
    a = rng.standard_normal((3, 3))
    d = pkg.dynamics(float(rng.uniform(0.5, 3.0)), a @ a.T + np.eye(3), com=rng.standard_normal(3) * 0.05, gravity_scale=float(rng.uniform(0, 2)),
                     force=rng.standard_normal(3), torque=rng.standard_normal(3), linear_damping=float(rng.uniform(0, 5)),
                     angular_damping=float(rng.uniform(0, 5)), confined=i % 10 != 9)
    return o, d, rng.standard_normal(6) * 0.01


def test_host_step_matches_the_restatement(pkg):
    sp = _rotated_params(pkg)
    A, half = pkg.rotation_mat3(list(sp.param_boxEulerDeg)), pkg.effective_half(sp)
    W = S.world_of(pkg, sp)
    rng = np.random.default_rng(2024)
    dt = F(sp.param_timeStep)
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    cases = [_random_case(pkg, rng, sp, A, half, i) for i in range(200)]
    for i0 in range(0, 200, 8):                                            # sets of eight, with a kinematic body in every other set
        chunk = cases[i0:i0 + 8]
        arr = pkg.obstacle_array([c[0] for c in chunk])
        recs = [c[1] for c in chunk]
        if (i0 // 8) % 2:
            recs[3] = None
        imp = np.array([c[2] for c in chunk])
        got = pkg.obstacles_step_host(arr, recs, imp, sp, dt)
        darr = pkg.dynamics_array(recs)
        infos = []
        want = R.to_array(B.step_all(R.bodies(arr, normalise=False), [B.record(x) for x in darr], imp, W, dt, infos))
        same_bits(got, want, f"bodies {i0}..{i0 + 7}")
        for info in infos:
            seen[len(info["faces"])] = seen.get(len(info["faces"]), 0) + 1
    print(f"bodies by the number of faces they penetrate: {seen}")
    assert all(seen[k] >= 10 for k in (0, 1, 2, 3)), seen
    # null sums are zero sums
    arr = pkg.obstacle_array([c[0] for c in cases[:4]])
    same_bits(pkg.obstacles_step_host(arr, [c[1] for c in cases[:4]], None, sp, dt),
               pkg.obstacles_step_host(arr, [c[1] for c in cases[:4]], np.zeros((4, 6)), sp, dt), "null sums")


# ---- 3. known answers -------------------------------------------------------------------------------
def test_free_fall_without_fluid(pkg):
    sp = pkg.default_params()
    dt = F(sp.param_timeStep)
    arr = pkg.obstacle_array([pkg.obstacle(R.BOX, (0.5, 2.0, -1.0), (0.4, 0.2, 0.3), rotation=(0.9, 0.1, 0.3, 0.2), vel=(1.0, 0.0, -2.0))])
    arr = R.to_array(R.bodies(arr, normalise=True))
    d = pkg.dynamics_box(500.0, (0.4, 0.2, 0.3))
    push = F(dt * F(sp.param_gravityY))
    vy, ref = F(0), R.bodies(arr, normalise=False)
    for n in range(1, 41):
        arr = pkg.obstacles_step_host(arr, [d], None, sp, dt)
        vy = F(vy + push)                                                 # the n-fold rounded sum of dt g_y
        ref[0]["v"] = np.array([F(1.0), vy, F(-2.0)], F)
        ref = R.advance(ref, dt)                                          # center follows obs_advance with the new velocity
        assert arr["vel"][0][1] == vy, (n, arr["vel"][0], vy)
        same_bits(arr, R.to_array(ref), f"free fall, step {n}")
    assert vy < -30 * abs(float(push))


def test_a_body_nothing_acts_on_keeps_every_bit_of_its_pose(pkg):
    sp = _rotated_params(pkg, param_gravityY=0.0)
    arr = pkg.obstacle_array([pkg.obstacle(R.CAPSULE, (0.3, 0.1, -0.2), (0.3, 0.4), rotation=(0.7, -0.2, 0.5, 0.1)),
                              pkg.obstacle(R.BOX, (-0.4, 0.2, 0.5), (0.3, 0.2, 0.4), rotation=(0.3, 0.8, -0.1, 0.4)),
                              pkg.obstacle(R.SPHERE, (0.0, -0.5, 0.0), 0.4)])
    arr = R.to_array(R.bodies(arr, normalise=True))
    a = np.array([[2.0, 0.3, -0.2], [0.3, 1.5, 0.4], [-0.2, 0.4, 1.0]])
    recs = [pkg.dynamics(1.3, a, com=(0.02, -0.05, 0.01)), pkg.dynamics_box(700.0, (0.3, 0.2, 0.4)), pkg.dynamics_sphere(300.0, 0.4)]
    cur = arr
    for _ in range(25):
        cur = pkg.obstacles_step_host(cur, recs, np.zeros((3, 6)), sp, F(sp.param_timeStep))
    same_bits(cur, arr, "zero sums, no gravity, omega = 0")


@pytest.mark.parametrize("e", [0.0, 0.15, 0.5, 1.0])
def test_a_sphere_dropped_on_the_floor_leaves_with_minus_e_times_its_speed(pkg, e):
    """V' = v_n + (j / m), j = (-(1 + e) v_n) / (1 / m): four roundings of relative size 2^-24 in j / m (1 + e, the product, the quotient,
    the product with 1 / m) on a quantity of size (1 + e) |v_n|, and the final add: |V' + e v_n| <= 8 2^-24 (1 + e) |v_n| with room."""
    sp = pkg.default_params(param_wallRestitution=e)
    floor = float(sp.param_boxCenter[1]) - float(pkg.effective_half(sp)[1])
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, (1.0, floor + 0.5 - 1e-3, -2.0), 0.5, vel=(0.7, -3.0, 0.2), omega=(1.0, 2.0, 3.0))])
    d = pkg.dynamics_sphere(600.0, 0.5, gravity_scale=0.0)
    dt = F(sp.param_timeStep)
    got = pkg.obstacles_step_host(arr, [d], None, sp, dt)
    want = R.to_array(B.step_all(R.bodies(arr, normalise=False), [B.record(pkg.dynamics_array([d])[0])], None, S.world_of(pkg, sp), dt))
    same_bits(got, want, f"bounce, e = {e}")
    vy = float(got["vel"][0][1])
    print(f"e = {e}: V_y -3 -> {vy!r}")
    assert abs(vy - 3.0 * float(F(e))) <= 8 * U * (1 + e) * 3.0
    assert got["vel"][0][0] == F(0.7) and got["vel"][0][2] == F(0.2) and np.array_equal(got["omega"][0], arr["omega"][0])   # no tangential impulse
    assert got["center"][0][1] >= F(floor + 0.5)                          # moved inward by the penetration, then up


def test_a_body_resting_on_the_floor_stays_inside(pkg):
    """A sphere and an upright capsule at rest on an inelastic floor (param_wallRestitution = 0; with e > 0 the impulse rule of section 3g
    makes a body in contact leave the face with e |v_n| every substep, so it does not rest: a stated limit): touching counts as contact,
    gravity's dt g is taken out again by the impulse, and the height stays within one fp32 rounding of floor + R."""
    sp = pkg.default_params(param_wallRestitution=0.0)
    floor = float(sp.param_boxCenter[1]) - float(pkg.effective_half(sp)[1])
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, (1.0, floor + 0.5, -2.0), 0.5), pkg.obstacle(R.CAPSULE, (-2.0, floor + 0.75, 1.0), (0.25, 0.5))])
    recs = [pkg.dynamics_sphere(3000.0, 0.5), pkg.dynamics_capsule(3000.0, (0.25, 0.5))]
    dt = F(sp.param_timeStep)
    rest = arr["center"][:, 1].copy()
    worst = 0.0
    for _ in range(500):
        arr = pkg.obstacles_step_host(arr, recs, None, sp, dt)
        worst = max(worst, float(np.abs(arr["center"][:, 1].astype(np.float64) - rest).max()))
        assert (np.abs(arr["center"][:, 1].astype(np.float64) - rest) <= np.spacing(np.abs(rest))).all(), arr["center"]
    print(f"largest |y - (floor + R)| over 500 substeps: {worst:.3g} (one rounding: {np.spacing(np.abs(rest))})")
    assert np.isfinite(arr["vel"]).all() and (np.abs(arr["vel"]) < 1e-3).all()


# ---- 4. momentum ledger -----------------------------------------------------------------------------
def test_momentum_ledger(pkg, oracle):
    """Per substep and component, for bodies with com = 0, no damping and no contact:  V' = fl(fl(V + fl32(J / m)) + p),  p = fl(dt g) the
    fp32 product the engine forms once per substep from the constants dt and g (gravityScale 1, no force: the acceleration is g exactly).
    The three fp32 operations that form V' are the cast of J / m, the first add and the second add; each is off by at most half an ulp
    of its own result, so with X = max(|fl32(J / m)|, |V + J / m|, |V'|):
        | m (V' - V) - J - m p |  <=  m (1.5 ulp(X) + 2^-52 |J / m|)
    (the last term is the fp64 division).  The ledger takes gravity's momentum as m p, the engine's own product: measured against the
    exact dt g the rounding of that product, half an ulp of dt g, would be a fourth term that no operation on V' makes."""
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    op = to_oracle_params(oracle, sp)
    p = rec["pos"][rec["isGhost"] == 0][:, :3].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    c, E = 0.5 * (lo + hi), float((hi - lo).max())
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, c + E * np.array([-0.25, 0.1, 0.0]), 0.12 * E, omega=(1.0, 0.0, 2.0)),
                              pkg.obstacle(R.BOX, c + E * np.array([0.25, 0.0, 0.1]), (0.15 * E, 0.1 * E, 0.1 * E), rotation=(0.9, 0.2, 0.3, 0.1)),
                              pkg.obstacle(R.CAPSULE, c + E * np.array([0.0, -0.1, -0.25]), (0.1 * E, 0.1 * E), rotation=(0.8, -0.3, 0.1, 0.4))])
    arr = R.to_array(R.bodies(arr, normalise=True))
    rho = float(sp.param_restDensity)
    recs = [pkg.dynamics_sphere(0.5 * rho, 0.12 * E, confined=False), pkg.dynamics_box(0.8 * rho, (0.15 * E, 0.1 * E, 0.1 * E), confined=False),
            pkg.dynamics_capsule(2.0 * rho, (0.1 * E, 0.1 * E), confined=False)]
    dt = F(sp.param_timeStep)
    g = [F(sp.param_gravityX), F(sp.param_gravityY), F(sp.param_gravityZ)]
    push = np.array([float(F(dt * x)) for x in g])
    mass = np.array([float(d.mass) for d in recs])
    worst, pushed = 0.0, 0
    for k in range(50):
        rec = oracle.substep(rec, op, dt=-1.0)
        rec, J = pkg.obstacles_apply_host(arr, F(sp.param_mass), rec)
        new = pkg.obstacles_step_host(arr, recs, J, sp, dt)
        V, V1 = arr["vel"].astype(np.float64), new["vel"].astype(np.float64)
        jm32 = (J[:, :3] / mass[:, None]).astype(F)
        t1 = (arr["vel"] + jm32).astype(F)
        X = np.maximum(np.maximum(np.abs(jm32), np.abs(t1)), np.abs(new["vel"]))
        bound = mass[:, None] * (1.5 * np.spacing(X).astype(np.float64) + 2.0 ** -52 * np.abs(J[:, :3] / mass[:, None]))
        res = np.abs(mass[:, None] * (V1 - V) - J[:, :3] - mass[:, None] * push[None, :])
        worst = max(worst, float((res / bound).max()))
        pushed += int((J[:, :3] != 0).any(axis=1).sum())
        assert (res <= bound).all(), f"substep {k}: residual {res} above {bound}"
        arr = new
    print(f"largest residual / bound over 50 substeps: {worst:.3g}; body-substeps with a fluid impulse: {pushed} of 150")
    assert pushed >= 100


# ---- 5. floating ------------------------------------------------------------------------------------
def _run_floating(pkg, oracle, mode):
    """400 substeps of the floating scene: oracle.substep, then the obstacle step and the body step through the host entry points
    ("host") or through the restatements ("ref").  Returns heights, J_y per substep, M g dt, and the worst depth excess."""
    rec, sp, arr, dyn = S.floating_scene(pkg)
    op = to_oracle_params(oracle, sp)
    dt = F(sp.param_timeStep)
    W = S.world_of(pkg, sp)
    ds = [B.record(x) for x in pkg.dynamics_array(dyn)]
    bs = R.bodies(arr, normalise=True)
    arr = R.to_array(bs)
    H, JY, excess = [], [], -1.0
    for _ in range(S.FLOAT_STEPS):
        rec = oracle.substep(rec, op, dt=-1.0)
        if mode == "host":
            rec, imp = pkg.obstacles_apply_host(arr, F(sp.param_mass), rec)
            arr = pkg.obstacles_step_host(arr, dyn, imp, sp, dt)
            before, bs = bs, R.bodies(arr, normalise=False)
            assert np.isfinite(imp).all() and all(np.isfinite(arr[f]).all() for f in ("center", "rotation", "vel", "omega")), "a record is not finite"
            p = rec["pos"][rec["isGhost"] == 0][:, :3]
            for b0, b1 in zip(before, bs):
                excess = max(excess, float(S.depth(b1, p).max()) - S.depth_allowance(b0, b1, p, dt))
        else:
            rec, imp, _ = R.apply(bs, F(sp.param_mass), rec)
            bs = B.step_all(bs, ds, imp, W, dt)
        H.append([float(b["c"][1]) for b in bs])
        JY.append(imp[:, 1].copy())
    wdt = np.array([float(d.mass) for d in dyn]) * abs(float(sp.param_gravityY)) * float(dt)
    floor = float(sp.param_boxCenter[1]) - float(pkg.effective_half(sp)[1])
    return np.array(H), np.array(JY), wdt, excess, floor


def test_floating(pkg, oracle):
    """Three spheres of radius 0.5 and 0.2 / 0.6 / 3.0 times the rest density dropped into the settled pool, 400 substeps through
    sph_obstacles_apply_host + sph_obstacles_step_host, against the same run through obstacle_ref + body_ref (the two differ in the order of
    the fp64 impulse sums only, so their trajectories drift apart by last bits; long trajectories are compared by what they mean).

    * Mean heights over the last 100 substeps are ordered, each gap at least half the restatement's own gap.  The restatement reaches
      -5.906 / -6.182 / -6.500: gaps 0.276 and 0.318.
    * The heavy sphere sits at floor + R to one fp32 rounding of that height (the bound of the resting test).  The scene runs with
      param_wallRestitution = 0 for that: with the default 0.15 the impulse rule makes the sunk sphere leave the floor with 0.15 |v_n|
      every other substep and fall back through it by dt |V|, and its mean height is then 1.4e-4 BELOW floor + R.
    * The fluid carries the floaters' weight: mean J_y / (M g dt) over the tail against the restatement's value, within three times the
      largest difference between the means of any two 100-substep windows inside substeps 200-400 of the restatement's run.  Measured on the
      restatement: shares 0.993 / 0.997, margins 0.046 / 0.030.
    * Every record finite; no particle deeper inside a body after the substep than dt (|V| + |omega| r_max) plus the rounding term of
      section 3e, V and omega the velocities the body left the substep with: the particles left the pass on the entry pose's surface and
      the pose then moved by dt V.  In a substep in which the container contact also shifted the centre, the shift is part of that motion
      (body_scenes.depth_allowance takes |c' - c| for dt |V|; with dt |V| alone the substep in which the sunk sphere is put back onto
      the floor misses by the 2.2e-3 it had fallen through)."""
    H, JY, wdt, excess, floor = _run_floating(pkg, oracle, "host")
    rH, rJY, _, _, _ = _run_floating(pkg, oracle, "ref")
    h, ratio, _ = S.floating_measures(H, JY, wdt)
    rh, rratio, rwin = S.floating_measures(rH, rJY, wdt)
    S.check_floating(h, ratio, rh, rratio, rwin, floor, "host entry points")
    rest = floor + S.FLOAT_R
    print(f"heavy sphere: mean height {h[2]!r}, floor + R = {rest}; worst depth minus allowance {excess:.3g}")
    assert abs(h[2] - rest) <= np.spacing(F(abs(rest)))
    assert excess <= 0.0


# ---- 6. moments -------------------------------------------------------------------------------------
def _torus(R0, r0, nu=32, nv=16, center=(0.0, 0.0, 0.0)):
    """A torus about the y axis, counter-clockwise seen from outside."""
    u = np.arange(nu) * 2 * np.pi / nu
    v = np.arange(nv) * 2 * np.pi / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    x = (R0 + r0 * np.cos(vv)) * np.cos(uu)
    z = (R0 + r0 * np.cos(vv)) * np.sin(uu)
    y = r0 * np.sin(vv)
    verts = (np.stack([x, y, z], axis=-1).reshape(-1, 3) + np.asarray(center)).astype(F)
    tris = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            tris += [(a, b, c), (a, c, d)]
    tris = np.array(tris, np.uint32)
    if _mesh_moments(verts, tris)[0] < 0:
        tris = tris[:, ::-1].copy()
    return verts, tris


def _mesh_moments(v, t):
    """fp64 volume and centroid of a closed mesh (signed tetrahedra from the origin)."""
    a, b, c = (v[t[:, k]].astype(np.float64) for k in range(3))
    vol6 = np.einsum("ij,ij->i", a, np.cross(b, c))
    vol = vol6.sum() / 6.0
    cen = ((a + b + c) * vol6[:, None]).sum(axis=0) / 24.0 / vol
    return vol, cen


def _mesh_lattice(pkg, v, t, h, margin=2.5):
    """A lattice of spacing h centred on the origin that covers the mesh with a margin of cells: (values, dims)."""
    ext = np.abs(v.astype(np.float64)).max(axis=0)
    dims = [2 * int(math.ceil(e / h + margin)) + 1 for e in ext]
    origin = [-(0.5 * (n - 1)) * h for n in dims]
    return pkg.mesh_distance_host(v, t, origin, h, dims)


def test_moments_of_mesh_lattices(pkg):
    """The volume bound: the weight w = clamp(0.5 - phi / D, 0, 1) of a lattice point is 1 where phi <= -D / 2 and 0 where phi >= D / 2.
    A point's cell (the box of one spacing about it) has half diagonal D / 2, so with exact distances it lies wholly inside the solid in
    the first case and wholly outside in the second, and w cell is the exact volume of solid in that cell.  Every other cell contributes an
    error of at most one cell volume: |V - V_mesh| <= cell #{|phi| < D / 2}.  For a first moment a wholly inside cell contributes
    x_i cell exactly (its centroid is the point), every other cell errs by at most cell (|x_i| + spacing / 2).  The centre of mass
    m_1 / m_0 then errs by at most (err_1 + |c| err_0) / m_0.  (The fp32 distances are off by a few 2^-24 of the scale, which moves a
    weight by that over D: far below one cell per boundary point.)"""
    for name, (v, t) in (("sphere", VR.icosphere(2, 0.8)), ("torus", _torus(0.7, 0.3)), ("shifted sphere", VR.icosphere(2, 0.7, center=(0.13, -0.21, 0.08)))):
        vol, cen = _mesh_moments(v, t)
        errs = []
        for h in (0.12, 0.06):
            values = _mesh_lattice(pkg, v, t, h)
            got = pkg.volume_moments_host(values, h)
            want, bound = B.moments(values, h)
            err = np.abs(got - want)
            assert (err <= bound).all(), f"{name} h={h}: |host - restatement| {err} above {bound}"
            terms, cell, diag = B.moment_terms(values, h)
            nb = int((np.abs(values.astype(np.float64)) < 0.5 * diag).sum())
            assert nb > 100 and abs(cell - h ** 3) < 1e-6 * h ** 3
            verr = abs(got[0] - vol)
            print(f"{name} h={h}: {values.size} points, volume {got[0]:.6f} against {vol:.6f}: error {verr:.3g}, bound {cell * nb:.3g} ({nb} boundary points)")
            assert verr <= cell * nb
            errs.append(verr)
            # the centre of mass
            nz, ny, nx = values.shape
            near = np.abs(values.astype(np.float64)) < 0.5 * diag
            coords = [VR.lattice_coords(n, h) for n in (nx, ny, nz)]
            grids = np.meshgrid(coords[2], coords[1], coords[0], indexing="ij")[::-1]   # x, y, z arrays of shape (nz, ny, nx)
            mass, com, inertia = pkg.mass_properties(got, 2.0)
            for a in range(3):
                e1 = cell * (np.abs(grids[a][near]) + 0.5 * h).sum()
                cb = (e1 + abs(cen[a]) * cell * nb) / got[0]
                assert abs(com[a] - cen[a]) <= cb, f"{name} h={h} axis {a}: centre of mass {com[a]} against {cen[a]}, bound {cb}"
            print(f"{name} h={h}: centre of mass {com} against {cen}")
            assert abs(mass - 2.0 * got[0]) <= 1e-12 * mass and (inertia[:3] > 0).all()
        assert errs[1] < errs[0], f"{name}: halving the spacing did not shrink the volume error: {errs}"
        if name == "shifted sphere":
            assert np.abs(cen).min() > 0.05 and np.abs(com - cen).max() < 0.01
    # a sphere's inertia through mass_properties: 2/5 m R^2 within the discretisation (1 %)
    values = VR.sphere_lattice(0.8, 0.05)
    mass, com, inertia = pkg.mass_properties(pkg.volume_moments_host(values, 0.05), 1.0)
    assert np.abs(inertia[:3] / (0.4 * mass * 0.64) - 1.0).max() < 0.01 and np.abs(inertia[3:]).max() < 1e-3 * inertia[0] and np.abs(com).max() < 1e-6


# ---- 7. refusals ------------------------------------------------------------------------------------
def test_refusals_of_the_host_step(pkg):
    L = pkg.load_library()
    sp = pkg.default_params()
    arr = pkg.obstacle_array([pkg.obstacle(R.BOX, (0, 0, 0), (0.4, 0.2, 0.3), vel=(1, 2, 3)), pkg.obstacle(R.SPHERE, (2, 0, 0), 0.5)])
    good = pkg.dynamics_box(500.0, (0.4, 0.2, 0.3))

    def bad(**kw):
        d = pkg.SphObstacleDynamics.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            cur = getattr(d, k)
            if hasattr(cur, "__len__"):
                cur[:] = v
            else:
                setattr(d, k, v)
        return d
    cases = {"mass 0 in a slot that must be dynamic is kinematic": None,
             "negative mass": bad(mass=-1.0), "nan mass": bad(mass=float("nan")), "inf force": bad(force=(0.0, float("inf"), 0.0)),
             "nan com": bad(com=(float("nan"), 0.0, 0.0)), "negative linear damping": bad(linearDamping=-0.1), "negative angular damping": bad(angularDamping=-1.0),
             "inertia with a negative diagonal": bad(inertia=(1.0, -1.0, 1.0, 0.0, 0.0, 0.0)), "singular inertia": bad(inertia=(1.0, 1.0, 1.0, 1.0, 0.0, 0.0)),
             "indefinite inertia": bad(inertia=(1.0, 1.0, 1.0, 0.9, 0.9, -0.9)), "nan torque": bad(torque=(0.0, 0.0, float("nan")))}
    for what, d in cases.items():
        if d is None:
            continue
        before = arr.copy()
        dyn = pkg.dynamics_array([good, d])
        rc = L.sph_obstacles_step_host(arr.ctypes.data_as(C.c_void_p), dyn.ctypes.data_as(C.c_void_p), 2, None, C.byref(sp), F(1e-3))
        assert rc == -1, what
        same_bits(arr, before, what + ": the bodies stay")
    dyn = pkg.dynamics_array([good, good])
    before = arr.copy()
    assert L.sph_obstacles_step_host(arr.ctypes.data_as(C.c_void_p), None, 2, None, C.byref(sp), F(1e-3)) == -1
    assert L.sph_obstacles_step_host(arr.ctypes.data_as(C.c_void_p), dyn.ctypes.data_as(C.c_void_p), 2, None, None, F(1e-3)) == -1
    assert L.sph_obstacles_step_host(arr.ctypes.data_as(C.c_void_p), dyn.ctypes.data_as(C.c_void_p), 17, None, C.byref(sp), F(1e-3)) == -1
    assert L.sph_obstacles_step_host(arr.ctypes.data_as(C.c_void_p), dyn.ctypes.data_as(C.c_void_p), 2, None, C.byref(sp), F(np.nan)) == -1
    same_bits(arr, before, "refused calls")
    out = np.full(10, 7.0)
    v = np.zeros((3, 3, 3), F)
    d3, s3 = (C.c_int * 3)(3, 3, 3), (C.c_float * 3)(0.1, 0.1, 0.1)
    assert L.sph_volume_moments_host(None, d3, s3, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.sph_volume_moments_host(v.ctypes.data_as(C.c_void_p), (C.c_int * 3)(3, 1, 3), s3, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.sph_volume_moments_host(v.ctypes.data_as(C.c_void_p), d3, (C.c_float * 3)(0.1, -0.1, 0.1), out.ctypes.data_as(C.c_void_p)) == -1
    assert (out == 7.0).all()
    # a NaN distance weighs nothing
    v = VR.sphere_lattice(0.3, 0.1)
    w = v.copy()
    w[0, 0, 0] = np.nan
    assert np.array_equal(pkg.volume_moments_host(v, 0.1), pkg.volume_moments_host(w, 0.1))
