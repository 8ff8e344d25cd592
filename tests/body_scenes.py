"""Scenes and measures shared by tests/test_bodies_cpu.py and tests/test_gpu_bodies.py (dynamic rigid bodies)."""
from __future__ import annotations

import math
import os

import numpy as np

import body_ref as B
import obstacle_ref as R

F = np.float32
U = 2.0 ** -24
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOAT_STEPS, FLOAT_TAIL = 400, 100
FLOAT_R = 0.5
FLOAT_DENSITIES = (0.2, 0.6, 3.0)                                         # times the rest density: floats high, floats low, sinks


def world_of(pkg, sp):
    return B.world((sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ), list(sp.param_boxCenter), pkg.rotation_mat3(list(sp.param_boxEulerDeg)),
                   pkg.effective_half(sp), sp.param_wallRestitution)


def depth(b, p):
    """fp64 depth of points p inside body b (<= 0 outside), on the body's own fp32 rotation matrix."""
    M = b["M"].astype(np.float64).reshape(3, 3)
    d = p.astype(np.float64) - b["c"].astype(np.float64)
    sz = b["size"].astype(np.float64)
    if b["shape"] == R.SPHERE:
        return sz[0] - np.sqrt((d * d).sum(axis=1))
    loc = d @ M
    if b["shape"] == R.BOX:
        return (sz[None, :] - np.abs(loc)).min(axis=1)
    s = np.clip(loc[:, 1], -sz[1], sz[1])
    e = loc.copy()
    e[:, 1] -= s
    return sz[0] - np.sqrt((e * e).sum(axis=1))


def r_max(b):
    sz = b["size"].astype(np.float64)
    if b["shape"] == R.SPHERE:
        return float(sz[0])
    if b["shape"] == R.BOX:
        return float(np.sqrt((sz * sz).sum()))
    return float(sz[0] + sz[1])


def depth_allowance(b0, b1, p, dt):
    """How deep a particle may lie inside body b1 (the pose after a substep) when the pass left it on the surface of b0 (the pose the
    substep began with): what the surface moved, |c1 - c0| + dt |omega| r_max, plus the rounding term of section 3e
    (tests/test_obstacles_cpu.py: 16 2^-24 (|p'| + extent)).  |c1 - c0| is dt |V| with V the velocity the body left the substep with,
    unless the container contact shifted the centre in this substep: then the shift is part of the motion."""
    dc = b1["c"].astype(np.float64) - b0["c"].astype(np.float64)
    w = b1["w"].astype(np.float64)
    return math.sqrt((dc * dc).sum()) + float(dt) * math.sqrt((w * w).sum()) * r_max(b1) + 16 * U * (float(np.abs(p).max()) + 2 * r_max(b1))


def floating_scene(pkg):
    """The settled pool with three spheres of radius 0.5 at x = -4, 0, 4 dropped from y = -5: (records, params, bodies, dynamics records).
    param_wallRestitution = 0, so that a sunk body can rest on the floor (test_bodies_cpu.test_floating says why)."""
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    sp = pkg.default_params(param_mass=float(fx["mass"]), param_wallRestitution=0.0)
    arr = pkg.obstacle_array([pkg.obstacle(R.SPHERE, (x, -5.0, 0.0), FLOAT_R) for x in (-4.0, 0.0, 4.0)])
    dyn = [pkg.dynamics_sphere(d * float(sp.param_restDensity), FLOAT_R) for d in FLOAT_DENSITIES]
    return fx["settled"], sp, arr, dyn


def floating_measures(heights, jy, weights_dt):
    """heights, jy: (steps, K).  Mean height over the tail, the fluid's mean J_y per substep over M g dt in the tail, and the same ratio
    in every 100-substep window inside substeps 200-400."""
    h = np.asarray(heights)[-FLOAT_TAIL:].mean(axis=0)
    jy = np.asarray(jy)
    ratio = jy[-FLOAT_TAIL:].mean(axis=0) / weights_dt
    windows = np.array([jy[s:s + 100].mean(axis=0) / weights_dt for s in range(200, 301)])
    return h, ratio, windows


def check_floating(h, ratio, ref_h, ref_ratio, ref_windows, floor_y, what):
    """The assertions of the floating scene against the restatement's own run (see test_bodies_cpu.test_floating for the derivations)."""
    print(f"{what}: heights {h} (restatement {ref_h}); fluid share of the weight {ratio} (restatement {ref_ratio})")
    assert h[0] > h[1] > h[2], f"{what}: heights not ordered {h}"
    assert h[0] - h[1] >= 0.5 * (ref_h[0] - ref_h[1]) and h[1] - h[2] >= 0.5 * (ref_h[1] - ref_h[2]), f"{what}: gaps {h[0] - h[1]}, {h[1] - h[2]}"
    margin = 3.0 * (ref_windows.max(axis=0) - ref_windows.min(axis=0))
    print(f"{what}: margins on the fluid's share {margin[:2]}")
    assert (np.abs(ratio[:2] - ref_ratio[:2]) <= margin[:2]).all(), f"{what}: share {ratio[:2]} against {ref_ratio[:2]} +- {margin[:2]}"
    return margin
