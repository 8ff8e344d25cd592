"""Kinematic solid obstacles without a GPU: the host entry points (sph_obstacles_apply_host / _advance_host, the same __host__ __device__
functions the kernels run) against the numpy restatement tests/obstacle_ref.py, the C layout of SphObstacle, and the example.

Bounds used below and where they come from:
* Impulses: the terms t_i are exactly defined, only the order of their fp64 sum is free.  Two sums of the same n
  terms in different orders differ by at most 2 (n - 1) 2^-53 sum |t_i| per component (each is within (n - 1) u sum |t_i| of the exact
  sum); the restatement's sum is the correctly rounded one (math.fsum).
* "Inside after one application": a projected position is c + M o rounded to fp32.  The final add rounds by half an ulp of |p'|, the
  dot3 of M o by about two ulps of |o|, and M is orthonormal to a few 2^-24; measured in fp64 on the same M, a projected particle lies
  at most 16 2^-24 (|p'| + extent) inside its body.
"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
import obstacle_ref as R
from support import build_example, c_layout, check_impulses, check_shim_syntax, records, same_bits

F = np.float32
U = 2.0 ** -24
OBSTACLE_SYMBOLS = ("sph_obstacle_default", "sph_obstacles_set", "sph_obstacles_set_motion", "sph_obstacles_get", "sph_obstacles_impulses",
                    "sph_obstacles_apply_host", "sph_obstacles_advance_host")


def _quat(rng):
    q = rng.standard_normal(4).astype(F)
    return R.normalize(q)


def _bodies(pkg, rng, shapes, centers, scale=1.0, spin=True):
    out = []
    for i, (shape, c) in enumerate(zip(shapes, centers)):
        if shape == R.SPHERE:
            size = (0.6 * scale,)
        elif shape == R.BOX:
            size = (0.5 * scale, 0.35 * scale, 0.25 * scale)
        else:
            size = (0.3 * scale, 0.4 * scale)
        w = rng.standard_normal(3) * 3.0 if spin and i % 2 == 0 else (0.0, 0.0, 0.0)
        out.append(pkg.obstacle(shape, c, size, rotation=_quat(rng), vel=rng.standard_normal(3), omega=w,
                                restitution=float(rng.uniform(0, 1)), friction=float(rng.uniform(0, 1))))
    return pkg.obstacle_array(out)


def test_library_exports_the_obstacle_interface(pkg):
    L = pkg.load_library()
    for name in OBSTACLE_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphObstacle) == 76 and pkg.OBSTACLE_DTYPE.itemsize == 76 and R.OBSTACLE_DTYPE == pkg.OBSTACLE_DTYPE
    assert (pkg.SPH_OBSTACLE_SPHERE, pkg.SPH_OBSTACLE_BOX, pkg.SPH_OBSTACLE_CAPSULE, pkg.SPH_MAX_OBSTACLES) == (R.SPHERE, R.BOX, R.CAPSULE, 16)
    eng = open(os.path.join(ROOT, PKG_NAME, "csrc", "sph_engine.hip")).read()
    assert "static_assert(sizeof(SphObstacle) == 76" in eng
    for m in ("set_obstacles", "set_obstacle_motion", "obstacles", "obstacle_impulses", "clear_obstacles"):
        assert hasattr(pkg.SPHFluidGPU, m), m
    d = pkg.SphObstacle()
    L.sph_obstacle_default(C.byref(d))
    assert (d.shape, d.size[0], list(d.rotation), d.restitution, d.friction) == (0, 1.0, [1.0, 0.0, 0.0, 0.0], F(0.15), F(0.02))
    o = pkg.obstacle(pkg.SPH_OBSTACLE_CAPSULE, (1, 2, 3), (0.5, 2.0))
    assert list(o.size) == [0.5, 2.0, 0.0] and list(o.center) == [1.0, 2.0, 3.0] and o.restitution == F(0.15) and o.friction == F(0.02)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_ctypes_mirror_matches_the_header(pkg, tmp_path):
    """sizeof and every offsetof of SphObstacle, printed by C99 compiled against the header."""
    size, offsets, extra = c_layout("SphObstacle", pkg.SphObstacle, [
        'printf("enum %d %d %d %d\\n", SPH_OBSTACLE_SPHERE, SPH_OBSTACLE_BOX, SPH_OBSTACLE_CAPSULE, SPH_MAX_OBSTACLES);'], tmp_path)
    assert size == 76
    assert len(offsets) == len(pkg.SphObstacle._fields_)
    for (name, val), (fname, _) in zip(offsets, pkg.SphObstacle._fields_):
        assert name == fname and val == getattr(pkg.SphObstacle, fname).offset == pkg.OBSTACLE_DTYPE.fields[fname][1], (name, val)
    assert len(extra) == 1 and extra[0].split() == ["enum", "0", "1", "2", "16"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stirred_tank_compiles_and_links_against_the_c_abi(pkg, tmp_path):
    check_shim_syntax()
    assert os.path.exists(build_example(pkg, "stirred_tank", tmp_path, werror=True))


def _degenerate_cases(pkg):
    """Bodies with identity rotation (so that local coordinates are exact) and particles on every special case of section 3e.
    Returns (bodies, pos, vel, ghost, expectations) with expectations a list of (particle index, expected pos, expected vel or None)."""
    c = np.array([0.25, -0.5, 0.75], F)
    bodies = pkg.obstacle_array([
        pkg.obstacle(R.SPHERE, c, 0.5, vel=(0.5, 0.0, 0.0)),
        pkg.obstacle(R.CAPSULE, c + F(3), (0.5, 1.0), omega=(0.0, 0.0, 0.0)),
        pkg.obstacle(R.BOX, c - F(3), (1.0, 1.0, 0.5)),
    ])
    sphere, caps, box = c, c + F(3), c - F(3)
    pos, vel, exp = [], [], []

    def add(p, v, want_p=None, want_v=None):
        pos.append(np.asarray(p, F))
        vel.append(np.asarray(v, F))
        exp.append((len(pos) - 1, None if want_p is None else np.asarray(want_p, F), want_v))
    add(sphere, (0.0, -1.0, 0.0), sphere + np.array([0, 0.5, 0], F))                     # exact centre: local +y
    add(sphere + np.array([0.5, 0, 0], F), (-1.0, 0.0, 0.0), sphere + np.array([0.5, 0, 0], F), "keep")   # exactly on the surface: outside
    add(caps + np.array([0, 0.25, 0], F), (0.0, 0.0, 0.0), caps + np.array([0.5, 0.25, 0], F))   # on the core segment: local +x
    add(caps + np.array([0, 1.25, 0], F), (0.0, 1.0, 0.0), None)                         # inside the cap, moving outwards: u_n >= 0
    add(caps + np.array([0.5, -0.5, 0], F), (0.0, 0.0, 0.0), None, "keep")                # on the cylinder surface: outside
    add(box, (0.0, 0.0, 1.0), box + np.array([0, 0, 0.5], F))                            # centre of a box: the z face is the nearest
    add(box + np.array([0.5, 0.5, 0.0], F), (0.0, 0.0, 0.0), box + np.array([1.0, 0.5, 0.0], F))   # x and y faces equidistant: x
    add(box + np.array([0.0, 0.5, 0.0], F), (0.0, 0.0, 0.0), box + np.array([0.0, 1.0, 0.0], F))
    add(box + np.array([-0.25, 0.0, 0.0], F), (0.0, 0.0, 0.0), box + np.array([-0.25, 0.0, 0.5], F))
    add(box + np.array([1.0, 0.0, 0.0], F), (5.0, 0.0, 0.0), box + np.array([1.0, 0, 0], F), "keep")   # exactly on a face: outside
    add(np.array([np.nan, sphere[1], sphere[2]], F), (1.0, 1.0, 1.0), None, "keep")      # NaN coordinate: untouched
    add(sphere, (1.0, 2.0, 3.0), sphere, "keep")                                          # a ghost at the centre: untouched
    ghost = np.zeros(len(pos), np.int32)
    ghost[-1] = 1
    return bodies, np.array(pos, F), np.array(vel, F), ghost, exp


def test_degenerate_cases_follow_the_contract(pkg):
    bodies, pos, vel, ghost, exp = _degenerate_cases(pkg)
    rec = records(pkg, pos, vel, ghost)
    got, imp = pkg.obstacles_apply_host(bodies, 0.02, rec)
    want, want_imp, info = R.apply(R.bodies(bodies, normalise=False), F(0.02), rec)
    same_bits(got, want, "host vs reference")
    for i, p, v in exp:
        if p is not None:
            assert np.array_equal(got["pos"][i, :3], p), (i, got["pos"][i, :3], p)
        if v == "keep":
            same_bits(got[i:i + 1], rec[i:i + 1], f"record {i} must keep its bits")
    assert (got["vel"][3] == rec["vel"][3]).all() and not np.array_equal(got["pos"][3], rec["pos"][3])   # u_n >= 0: projected, velocity kept
    assert got["vel"][0, 1] > rec["vel"][0, 1]                                            # the u_n < 0 branch
    check_impulses(imp, want_imp, info, "degenerate cases")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_apply_matches_the_reference(pkg, seed):
    rng = np.random.default_rng(seed)
    shapes = [R.SPHERE, R.BOX, R.CAPSULE, R.SPHERE, R.BOX, R.CAPSULE, R.BOX]
    centers = (rng.uniform(-1, 1, (len(shapes), 3)) * 0.8).astype(F)                    # overlapping bodies: later ones see earlier results
    bodies = _bodies(pkg, rng, shapes, centers, scale=1.2)
    n = 30000
    pos = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    vel = (rng.standard_normal((n, 3)) * 2).astype(F)
    ghost = (rng.random(n) < 0.03).astype(np.int32)
    pos[rng.choice(n, 20, replace=False), rng.integers(0, 3, 20)] = np.nan
    rec = records(pkg, pos, vel, ghost)
    mass = F(rng.uniform(0.01, 2))
    got, imp = pkg.obstacles_apply_host(bodies, mass, rec)
    want, want_imp, info = R.apply(R.bodies(bodies, normalise=False), mass, rec)
    same_bits(got, want, f"seed {seed}: host vs reference")
    assert (info["touched"] > 50).all() and (info["negative"] > 10).all() and (info["touched"] > info["negative"]).all(), info["touched"]
    check_impulses(imp, want_imp, info, f"seed {seed}")
    # particles that no body touches keep their bits
    moved = (got.view(np.uint8).reshape(n, 80) != rec.view(np.uint8).reshape(n, 80)).any(axis=1)
    touched = np.zeros(n, bool)
    p, v = rec["pos"][:, :3].astype(F).copy(), rec["vel"][:, :3].astype(F).copy()
    act = (rec["isGhost"] == 0) & np.isfinite(p).all(axis=1)
    for b in R.bodies(bodies, normalise=False):
        p, v, inside, _, _ = R.hit(b, mass, p, v, act)
        touched |= inside
    assert not (moved & ~touched).any() and moved.sum() > 0
    assert not moved[rec["isGhost"] != 0].any() and not moved[~np.isfinite(pos).all(axis=1)].any()


def _depth(b, p):
    """fp64 depth of points p inside body b (<= 0 outside), on the body's own fp32 rotation matrix."""
    M = b["M"].astype(np.float64).reshape(3, 3)
    d = p.astype(np.float64) - b["c"].astype(np.float64)
    sz = b["size"].astype(np.float64)
    if b["shape"] == R.SPHERE:
        return sz[0] - np.sqrt((d * d).sum(axis=1))
    loc = d @ M                                                           # l = M^T d
    if b["shape"] == R.BOX:
        return (sz[None, :] - np.abs(loc)).min(axis=1)
    s = np.clip(loc[:, 1], -sz[1], sz[1])
    e = loc.copy()
    e[:, 1] -= s
    return sz[0] - np.sqrt((e * e).sum(axis=1))


def test_no_particle_is_inside_after_one_application(pkg):
    rng = np.random.default_rng(11)
    shapes = [R.SPHERE, R.BOX, R.CAPSULE, R.BOX, R.CAPSULE, R.SPHERE]
    centers = np.array([[-3, 0, 0], [0, 0, 0], [3, 0, 0], [-3, 3, 0], [0, 3, 0], [3, 3, 0]], F)   # 3 apart: no two bodies overlap
    bodies = _bodies(pkg, rng, shapes, centers, scale=1.5)
    n = 40000
    pos = np.concatenate([centers[i] + rng.uniform(-1.2, 1.2, (n // 6, 3)) for i in range(6)]).astype(F)
    vel = rng.standard_normal(pos.shape).astype(F)
    rec = records(pkg, pos, vel)
    got, _ = pkg.obstacles_apply_host(bodies, F(0.1), rec)
    bs = R.bodies(bodies, normalise=False)
    p = got["pos"][:, :3]
    inside_before = 0
    for b in bs:
        ext = float(np.abs(b["size"]).max()) * 2
        tol = 16 * U * (float(np.abs(p).max()) + ext)
        dep = _depth(b, p)
        inside_before += int((_depth(b, pos) > 0).sum())
        print(f"shape {b['shape']}: deepest after {dep.max():.3g}, allowed {tol:.3g}")
        assert dep.max() <= tol
    assert inside_before > 3000


def test_host_advance_matches_the_reference(pkg):
    rng = np.random.default_rng(5)
    shapes = [R.SPHERE, R.BOX, R.CAPSULE] * 3
    arr = _bodies(pkg, rng, shapes, rng.uniform(-3, 3, (len(shapes), 3)).astype(F))
    arr["omega"][1] = 0.0                                                 # one resting rotation...
    arr["vel"][2] = 0.0
    arr["omega"][2] = (0.0, 0.0, -0.0)                                     # ...and one whose omega is a signed zero
    bs = R.bodies(arr, normalise=False)
    cur = arr.copy()
    for k, dt in enumerate([1e-3, 1e-3, 2.5e-4, 0.01, 0.05] * 4):
        cur = pkg.obstacles_advance_host(cur, dt)
        bs = R.advance(bs, dt)
        want = R.to_array(bs)
        same_bits(cur, want, f"advance {k}")
    same_bits(cur["rotation"][1], arr["rotation"][1], "omega = 0 keeps the rotation bits")
    same_bits(cur["rotation"][2], arr["rotation"][2], "omega = -0 keeps the rotation bits")
    same_bits(cur["center"][2], arr["center"][2], "V = 0 keeps the centre bits")
    assert not np.array_equal(cur["rotation"][0], arr["rotation"][0])
    q = cur["rotation"].astype(np.float64)
    assert np.abs((q * q).sum(axis=1) - 1).max() < 8 * U


def test_refusals_of_the_host_entry_points(pkg):
    L = pkg.load_library()
    good = pkg.obstacle(R.BOX, (0, 0, 0), (1, 1, 1))
    rec = records(pkg, np.zeros((4, 3), F), np.zeros((4, 3), F))
    cases = []
    for field, val in (("shape", 3), ("shape", -1)):
        o = pkg.obstacle(R.BOX, (0, 0, 0), (1, 1, 1))
        setattr(o, field, val)
        cases.append(o)
    for mut in (lambda o: o.size.__setitem__(1, 0.0), lambda o: o.size.__setitem__(2, -1.0), lambda o: o.size.__setitem__(0, float("inf")),
                lambda o: [o.rotation.__setitem__(i, 0.0) for i in range(4)], lambda o: o.rotation.__setitem__(2, float("nan")),
                lambda o: [o.rotation.__setitem__(i, 1e30) for i in range(4)], lambda o: [o.rotation.__setitem__(i, 1e-30) for i in range(4)],
                lambda o: o.center.__setitem__(0, float("nan")), lambda o: o.vel.__setitem__(1, float("inf")), lambda o: o.omega.__setitem__(2, float("nan")),
                lambda o: setattr(o, "restitution", 1.5), lambda o: setattr(o, "friction", -0.1), lambda o: setattr(o, "friction", float("nan"))):
        o = pkg.obstacle(R.BOX, (0, 0, 0), (1, 1, 1))
        mut(o)
        cases.append(o)
    for o in cases:
        arr = pkg.obstacle_array([good, o])
        before = rec.copy()
        assert L.sph_obstacles_apply_host(arr.ctypes.data_as(C.c_void_p), 2, 1.0, rec.ctypes.data_as(C.c_void_p), len(rec), None) == -1
        assert L.sph_obstacles_advance_host(arr.ctypes.data_as(C.c_void_p), 2, 1e-3) == -1
        same_bits(rec, before, "a refused call writes nothing")
    # sizes a shape does not use are not checked for positivity; 17 bodies are too many
    sph = pkg.obstacle(R.SPHERE, (0, 0, 0), 1.0)
    arr = pkg.obstacle_array([sph])
    assert L.sph_obstacles_apply_host(arr.ctypes.data_as(C.c_void_p), 1, 1.0, rec.ctypes.data_as(C.c_void_p), len(rec), None) == 0
    many = pkg.obstacle_array([sph] * 17)
    assert L.sph_obstacles_advance_host(many.ctypes.data_as(C.c_void_p), 17, 1e-3) == -1
