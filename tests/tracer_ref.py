"""Numpy restatement of the passive tracers (include/sph_abi.h "passive tracers").

field(): the sampler's Shepard velocity u(x) and fraction phi(x) in the sampler's own fp32 arithmetic over the candidates of
oracle.build_grid's cells in canonical order (sample_ref.candidates): per candidate w = ((t t) t) invRho, wsum += w,
vx = fma(w, v_j.x, vx), then ONE fp32 division vx / wsum; zero where wsum = 0 or the point is not finite.
advect(): one substep of section 3d on a frozen state.  run(): n substeps, the state advanced by oracle.substep in between.
history_*(): the ring arithmetic of the pathline history.

fma is oracle._fma (the product is exact in float64) with the one case repaired in which rounding to float64 first and to fp32
second differs from a single rounding, so the restatement is exact and not only exact in all but 2^-29 of the cases.
"""
from __future__ import annotations

import numpy as np

import sample_ref

F = np.float32
EULER, MIDPOINT = 0, 1
TRACER_DTYPE = np.dtype([("pos", "<f4", (3,)), ("age", "<f4"), ("vel", "<f4", (3,)), ("fraction", "<f4")])


def _fma(a, b, c):
    """Correctly rounded fp32 fma of fp32 arrays (normal range)."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)          # exact: 24 + 24 bits
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p                                                          # TwoSum: s + err = p + c exactly
    err = (p - (s - bb)) + (c - bb)
    bits = np.atleast_1d(s).view(np.uint64)
    tie = ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (np.atleast_1d(err) != 0) & np.isfinite(np.atleast_1d(s))
    if tie.any():                                                       # s sits on an fp32 midpoint that the exact sum does not
        s = np.atleast_1d(s).copy()
        e = np.atleast_1d(err)
        s[tie] = np.nextafter(s[tie], np.where(e[tie] > 0, np.inf, -np.inf))
        s = s.reshape(np.shape(p))
    return np.asarray(s).astype(F)


def _dot3(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, (ax * bx).astype(F)))


def field(rec, points, h, mass, grid, cell_start, order):
    """(u (m, 3), phi (m,), n (m,), vmax (m,)): velocity and fraction of sph_sample_points at the points, the number of candidates with
    w > 0 and the largest |v_j| among them (float64)."""
    pts = np.asarray(points, F)[:, :3]
    m = len(pts)
    fin = np.isfinite(pts).all(axis=1)
    safe = np.where(fin[:, None], pts, F(0)).astype(F)
    idx = sample_ref.candidates(safe, grid, cell_start, order) if len(rec) else np.zeros((m, 0), np.int64)
    h2, mp6 = sample_ref.simk_consts(h, mass)
    pos = rec["pos"][:, :3].astype(F)
    vel = rec["vel"][:, :3].astype(F)
    rho = rec["density"].astype(F)
    inv = np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(F)
    wsum = np.zeros(m, F)
    acc = np.zeros((m, 3), F)
    npos = np.zeros(m, np.int64)
    vmax = np.zeros(m, np.float64)
    speed = np.sqrt((vel.astype(np.float64) ** 2).sum(axis=1))
    for k in range(idx.shape[1]):
        j = idx[:, k]
        ok = j >= 0
        if not ok.any():
            continue
        jj = np.where(ok, j, 0)
        d = (safe - pos[jj]).astype(F)
        r2 = _dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
        t = np.maximum(F(h2) - r2, F(0)).astype(F)
        w = (((t * t).astype(F) * t).astype(F) * inv[jj]).astype(F)
        wsum = np.where(ok, (wsum + w).astype(F), wsum)
        for a in range(3):
            acc[:, a] = np.where(ok, _fma(w, vel[jj, a], acc[:, a]), acc[:, a])
        npos += (ok & (w > 0)).astype(np.int64)
        vmax = np.where(ok & (w > 0), np.maximum(vmax, speed[jj]), vmax)
    any_w = fin & (wsum > 0)
    den = np.where(any_w, wsum, F(1)).astype(F)
    u = np.where(any_w[:, None], (acc / den[:, None]).astype(F), F(0)).astype(F)
    phi = np.where(fin, (F(mp6) * wsum).astype(F), F(0)).astype(F)
    return u, phi, np.where(fin, npos, 0), np.where(fin, vmax, 0.0)


def advect(tr, rec, h, mass, grid, cell_start, order, dt, integrator):
    """One substep of section 3d on the frozen state `rec`: a new TRACER_DTYPE array."""
    dt = F(dt)
    x = tr["pos"].astype(F)
    fin = np.isfinite(x).all(axis=1)
    u, phi, _, _ = field(rec, x, h, mass, grid, cell_start, order)
    v = u
    if integrator == MIDPOINT:
        hd = F(F(0.5) * dt)
        with np.errstate(all="ignore"):
            xm = (x + (hd * u).astype(F)).astype(F)
        v, _, _, _ = field(rec, xm, h, mass, grid, cell_start, order)
    out = tr.copy()
    with np.errstate(all="ignore"):
        moved = (x + (dt * v).astype(F)).astype(F)
    out["pos"] = np.where(fin[:, None], moved, x)                       # (non-finite tracers keep their position BITS: copies only)
    out["vel"] = np.where(fin[:, None], v, F(0))
    out["fraction"] = np.where(fin, phi, F(0))
    out["age"] = (tr["age"].astype(F) + dt).astype(F)
    return out


def seed(points):
    pts = np.asarray(points, F)
    tr = np.zeros(len(pts), TRACER_DTYPE)
    tr["pos"] = pts[:, :3]
    if pts.shape[1] > 3:
        tr["age"] = pts[:, 3]
    return tr


def step_on(oracle, rec, op, tr, dt, integrator):
    b = oracle.build_grid(rec, op)
    return advect(tr, rec, op.h, op.mass, b["grid"], b["cell_start"], b["order"], dt, integrator)


def run(oracle, rec, op, points, n, integrator, dt=None, snapshots=None):
    """n substeps: tracers advected on each substep's entry state, the state advanced by oracle.substep.  Returns (tracers, records);
    `snapshots`, a list, receives (x, y, z, age) after every substep (the seed first)."""
    tr = seed(points)
    step = F(op.timeStep if dt is None or dt <= 0 else dt)
    if snapshots is not None:
        snapshots.append(snapshot_of(tr))
    for _ in range(n):
        tr = step_on(oracle, rec, op, tr, step, integrator)
        rec = oracle.substep(rec, op, dt=float(step) if dt is not None and dt > 0 else -1.0)
        if snapshots is not None:
            snapshots.append(snapshot_of(tr))
    return tr, rec


def snapshot_of(tr):
    return np.concatenate([tr["pos"], tr["age"][:, None]], axis=1).astype(F)


# ---- pathline history: snapshot q after substep c = q S, in slot q mod K; the min(c / S + 1, K) newest are stored ----
def history_slot(q, K):
    return q % K


def history_stored(c, S, K):
    """(count, first): how many snapshots a download returns after c substeps, and the number of the oldest one."""
    if K == 0:
        return 0, 0
    last = c // S
    count = min(last + 1, K)
    return count, last + 1 - count


def history_write_slot(c_after, S, K):
    """Ring slot the substep that makes the counter c_after writes, or None."""
    if K == 0 or c_after % S:
        return None
    return history_slot(c_after // S, K)
