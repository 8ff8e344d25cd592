"""Passive tracers without a GPU: the library exports the interface, and the numpy restatement (tests/tracer_ref.py) against itself and
against facts that follow from DESIGN.md section 3d.

Bounds used below and where they come from:
* The Shepard velocity is a convex combination of the candidates' velocities (w_j >= 0), so |v| <= max{|v_j| : w_j > 0}; the fp32 sums and
  the division add a few 2^-24 relative per candidate (1e-5 covers several hundred candidates), and x + dt v rounds each coordinate
  to half an ulp of the position: |x' - x| <= dt max|v_j| (1 + 1e-5) + sqrt(3) ulp(max |x|).
* Equal velocities V: every product w V and every partial sum carries one rounding, the division one more: (n + 2) 2^-24 |V| per axis.
* Rigid rotation by theta = omega dt per step: Euler multiplies the radius by sqrt(1 + theta^2), the midpoint rule by
  sqrt(1 + theta^4 / 4); theta = 2 pi / 64 over 64 steps gives 1.36 and 1.0007.  The Shepard field is a smoothed omega x r; the numpy
  loop scattered by 1.345 ... 1.374 and 0.9942 ... 1.0067 when this was written, the test allows 3 % and 1 %.
"""
import ctypes as C
import os

import numpy as np

from conftest import ROOT, small_scene, to_oracle_params
import tracer_ref as T

F = np.float32
G = os.path.join(ROOT, "tests", "golden")
TRACER_SYMBOLS = ("sph_tracers_set", "sph_tracers_set_device", "sph_tracers_count", "sph_tracers_info", "sph_tracers_download",
                  "sph_tracers_device", "sph_tracers_history")


def test_library_exports_the_tracer_interface(pkg):
    L = pkg.load_library()
    for name in TRACER_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphTracer) == 32 and pkg.TRACER_DTYPE.itemsize == 32 and T.TRACER_DTYPE == pkg.TRACER_DTYPE
    assert [pkg.TRACER_DTYPE.fields[f][1] for f in ("pos", "age", "vel", "fraction")] == [0, 12, 16, 28]
    assert (pkg.SPH_TRACER_EULER, pkg.SPH_TRACER_MIDPOINT) == (0, 1) == (T.EULER, T.MIDPOINT)
    src = open(os.path.join(ROOT, "include", "sph_abi.h")).read()
    assert "typedef struct SphTracer { float pos[3]; float age; float vel[3]; float fraction; } SphTracer;" in src
    eng = open(os.path.join(ROOT, pkg.__name__, "csrc", "sph_engine.hip")).read()
    assert "static_assert(sizeof(SphTracer) == 32" in eng                 # the C side of the same fact, checked when the library is built
    for m in ("set_tracers", "tracers", "tracers_device", "tracer_history", "clear_tracers"):
        assert hasattr(pkg.SPHFluidGPU, m), m


def test_fma_of_the_restatement_is_correctly_rounded(oracle):
    # a b = 2^-24 + 2^-70 exactly (2^46 + 1 = 8392705 * 8384513): 1 + a b lies just ABOVE the midpoint of 1 and 1 + 2^-23, float64 drops the 2^-70
    a, b = F(8392705.0 * 2.0 ** -35), F(8384513.0 * 2.0 ** -35)
    assert float(a) * float(b) == 2.0 ** -24 + 2.0 ** -70
    assert T._fma(np.array([a]), np.array([b]), np.array([F(1)]))[0] == F(1 + 2.0 ** -23)
    assert T._fma(np.array([-a]), np.array([b]), np.array([F(-1)]))[0] == F(-1 - 2.0 ** -23)
    assert oracle._fma(np.array([a]), np.array([b]), np.array([F(1)]))[0] == F(1)       # (the double rounding this repairs)
    rng = np.random.default_rng(5)
    x, y, z = (rng.standard_normal(100000).astype(F) for _ in range(3))
    same = T._fma(x, y, z).view(np.uint32) == oracle._fma(x, y, z).view(np.uint32)
    assert same.mean() > 0.9999                                          # elsewhere the two agree


def _pool(pkg, oracle):
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    sp = pkg.default_params(param_mass=float(fx["mass"]))
    return fx["settled"], sp, to_oracle_params(oracle, sp)


def _pool_seeds(rec, rng, m=512):
    lo = rec["pos"][:, :3].min(axis=0) - F(0.5)
    hi = rec["pos"][:, :3].max(axis=0) + F(0.5)
    return (lo + (hi - lo) * rng.random((m, 3))).astype(F)


def test_step_is_bounded_by_the_fastest_candidate_and_dry_tracers_rest(pkg, oracle):
    rec, sp, op = _pool(pkg, oracle)
    rng = np.random.default_rng(21)
    pts = _pool_seeds(rec, rng)
    dt = F(sp.param_timeStep)
    for integ in (T.EULER, T.MIDPOINT):
        tr = T.seed(pts)
        state = rec
        ages = np.zeros(len(pts), F)
        moved_any = np.zeros(len(pts), bool)
        dry_always = np.ones(len(pts), bool)
        for _ in range(8):
            b = oracle.build_grid(state, op)
            args = (state, None, sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"])
            x = tr["pos"].copy()
            u, phi, n1, vmax = T.field(args[0], x, *args[2:])
            if integ == T.MIDPOINT:
                xm = (x + (F(F(0.5) * dt) * u).astype(F)).astype(F)
                _, _, _, vmax = T.field(args[0], xm, *args[2:])
            new = T.advect(tr, state, sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"], dt, integ)
            step = np.sqrt(((new["pos"].astype(np.float64) - x.astype(np.float64)) ** 2).sum(axis=1))
            ulp = np.spacing(np.maximum(np.abs(x).max(axis=1), np.abs(new["pos"]).max(axis=1)).astype(F)).astype(np.float64)
            bound = float(dt) * vmax * (1 + 1e-5) + np.sqrt(3.0) * ulp
            assert np.all(step <= bound), (integ, float((step - bound).max()))
            dry = n1 == 0                                                # sum w_j = 0: does not move, bit for bit
            assert np.array_equal(new["pos"][dry].view(np.uint32), x[dry].view(np.uint32))
            assert not new["vel"][dry].any() and not new["fraction"][dry].any()
            assert np.array_equal(new["fraction"], phi)                  # the fraction BEFORE the move
            ages = (ages + dt).astype(F)
            assert np.array_equal(new["age"], ages)                      # the fp32 running sum of dt
            moved_any |= (new["pos"] != x).any(axis=1)
            dry_always &= dry
            tr = new
            state = oracle.substep(state, op)
        assert moved_any.sum() > 200 and dry_always.sum() > 50, (moved_any.sum(), dry_always.sum())


def test_non_finite_tracers_keep_their_bits_and_age(pkg, oracle):
    rec, sp, op = _pool(pkg, oracle)
    pts = np.zeros((6, 4), F)
    pts[:, :3] = rec["pos"][:6, :3]
    pts[:, 3] = F(0.25)
    pts[0, 0] = np.nan
    pts[1, 1] = np.inf
    pts[2, 2] = -np.inf
    pts[3, :3] = np.nan
    for integ in (T.EULER, T.MIDPOINT):
        tr, _ = T.run(oracle, rec, op, pts, 3, integ)
        bad = slice(0, 4)
        assert np.array_equal(tr["pos"][bad].view(np.uint32), pts[bad, :3].view(np.uint32))
        assert not tr["vel"][bad].any() and not tr["fraction"][bad].any()
        want = F(0.25)
        for _ in range(3):
            want = F(want + F(sp.param_timeStep))
        assert np.all(tr["age"] == want)
        assert np.all(tr["fraction"][4:] > 0)


def test_uniform_velocity_is_reproduced(pkg, oracle):
    rec, sp, op = _pool(pkg, oracle)
    rec = rec.copy()
    V = np.array([1.25, -0.375, 2.0625], F) * F(1.1)
    rec["vel"][:, :3] = V
    b = oracle.build_grid(rec, op)
    pts = _pool_seeds(rec, np.random.default_rng(2), 400)
    u, phi, n, _ = T.field(rec, pts, sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"])
    wet = n > 0
    assert wet.sum() > 200
    tol = (n[wet, None] + 2) * 2.0 ** -24 * np.abs(V.astype(np.float64))[None, :]
    assert np.all(np.abs(u[wet].astype(np.float64) - V.astype(np.float64)[None, :]) <= tol)
    assert not u[~wet].any()


def test_midpoint_beats_euler_on_a_rigid_rotation(pkg, oracle):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    op = to_oracle_params(oracle, sp)
    rec = oracle.substep(rec, op)                                        # the records carry densities now
    pos = rec["pos"][:, :3].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    dt = F(sp.param_timeStep)
    omega = 2.0 * np.pi / 64.0 / float(dt)
    r = pos - centre
    rec["vel"][:, 0] = (-omega * r[:, 1]).astype(F)                      # omega z^ x r
    rec["vel"][:, 1] = (omega * r[:, 0]).astype(F)
    rec["vel"][:, 2] = 0
    radius = 0.25 * float((hi - lo)[:2].mean())
    ang = 2.0 * np.pi * np.arange(32) / 32.0
    pts = np.stack([centre[0] + radius * np.cos(ang), centre[1] + radius * np.sin(ang), np.full(32, centre[2])], axis=1).astype(F)
    b = oracle.build_grid(rec, op)
    assert float(sp.param_h) * 1.5 < 0.25 * half.min()                  # inside the inner 75 % means more than 1.5 h inside the block
    for integ, want, tol in ((T.EULER, (1.0 + (2 * np.pi / 64) ** 2) ** 32, 0.03), (T.MIDPOINT, 1.0, 0.01)):
        tr = T.seed(pts)
        for _ in range(64):                                              # a full turn on the one frozen state
            tr = T.advect(tr, rec, sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"], dt, integ)
            assert np.all(np.abs(tr["pos"].astype(np.float64) - centre) <= 0.75 * half), integ
        r0 = np.sqrt(((pts[:, :2] - centre[:2]) ** 2).sum(axis=1))
        r1 = np.sqrt(((tr["pos"][:, :2].astype(np.float64) - centre[:2]) ** 2).sum(axis=1))
        ratio = r1 / r0
        print("integrator", integ, "radius ratio", ratio.min(), ratio.max())
        assert np.all(np.abs(ratio / want - 1.0) <= tol), (integ, ratio.min(), ratio.max())
    assert abs((1.0 + (2 * np.pi / 64) ** 2) ** 32 - 1.36) < 0.005


def test_records_without_a_density_carry_nothing(pkg, oracle):
    """density <= 0 (spawned, synthetic or uploaded records before their first substep) means 1/rho = 0: u = 0 and fraction = 0, so
    tracers rest during the FIRST substep on such a state and move from the second on."""
    spawned, _ = pkg.spawn_particles(pkg.default_params(), 2000, seed=3)
    assert not spawned["density"].any()                                  # what sph_spawn_particles writes
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    assert not rec["density"].any()
    op = to_oracle_params(oracle, sp)
    rec = rec.copy()
    rec["vel"][:, :3] = F(1.5)
    pts = rec["pos"][::16, :3].copy()
    b = oracle.build_grid(rec, op)
    u, phi, n, _ = T.field(rec, pts, sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"])
    assert not u.any() and not phi.any() and not n.any()
    snaps = []
    tr, _ = T.run(oracle, rec, op, pts, 2, T.MIDPOINT, snapshots=snaps)
    assert np.array_equal(snaps[1][:, :3].view(np.uint32), pts.view(np.uint32))       # first substep: at rest
    assert (snaps[2][:, :3] != pts).any(axis=1).all()                    # second substep: carried along
    assert np.all(tr["fraction"] > 0)


def test_history_bookkeeping():
    for K in range(0, 6):
        for S in range(1, 5):
            ring = {}
            if K:
                ring[T.history_slot(0, K)] = 0                           # the seed
            for c in range(0, 40):
                if c:
                    slot = T.history_write_slot(c, S, K)
                    assert (slot is not None) == (K > 0 and c % S == 0)
                    if slot is not None:
                        assert 0 <= slot < K
                        ring[slot] = c // S
                count, first = T.history_stored(c, S, K)
                if K == 0:
                    assert (count, first) == (0, 0)
                    continue
                assert count == min(c // S + 1, K) and first + count - 1 == c // S
                assert sorted(ring.values())[-count:] == list(range(first, first + count))
                assert [ring[T.history_slot(q, K)] for q in range(first, first + count)] == list(range(first, first + count))
