"""Numpy restatement of the secondary particles (include/sph_abi.h "spray, foam and bubbles").

sample(): u and n of the sampler at the records' positions (tracer_ref.field for the Shepard velocity, sample_ref.emulate for the count).
step(): one substep of section 3j from those samples and the entry state: advance, spawn, order, totals.  Every fp32 expression is a
multiply and then an add, each rounded (numpy float32 arithmetic), in the order section 3j writes them.
scene() / scene_reference(): the shared scene of the CPU and GPU tests, run once per capacity by oracle.substep, sample() and step().
"""
from __future__ import annotations

import numpy as np

import sample_ref
import tracer_ref

F = np.float32
U32 = np.uint32
SPRAY, FOAM, BUBBLE = 0, 1, 2
DIFFUSE_DTYPE = np.dtype([("pos", "<f4", (3,)), ("life", "<f4"), ("vel", "<f4", (3,)), ("age", "<f4"),
                          ("parent", "<u4"), ("birth", "<u4"), ("kind", "<u4"), ("pad", "<u4")])
TOTALS = ("spawned", "dropped", "diedLife", "diedAge", "leftBox", "nonFinite")


def mix(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def hash32(seed, ids, c, draw):
    """The counter-based hash of (seed, id, 64-bit substep counter c, draw index) as uint32."""
    h = mix((int(seed) + 0x9e3779b9) & 0xFFFFFFFF)
    h = mix(h ^ np.asarray(ids, np.uint64))
    h = mix(h ^ np.uint64(int(c) & 0xFFFFFFFF))
    h = mix(h ^ np.uint64((int(c) >> 32) & 0xFFFFFFFF))
    return mix(h ^ np.asarray(draw, np.uint64)).astype(U32)


def uniform(seed, ids, c, draw):
    return ((hash32(seed, ids, c, draw) >> U32(8)).astype(F) * F(2.0 ** -24)).astype(F)


def empty():
    return np.zeros(0, DIFFUSE_DTYPE)


def new_totals():
    t = {k: 0 for k in TOTALS}
    t.update(substeps=0, seeded=0, alive=0, aliveByKind=[0, 0, 0])
    return t


def sample(rec, pos, h, mass, grid, cell_start, order):
    """(u (m, 3) float32, n (m,) uint32) of sph_sample_points at the positions."""
    if len(pos) == 0:
        return np.zeros((0, 3), F), np.zeros(0, U32)
    u, _, _, _ = tracer_ref.field(rec, pos, h, mass, grid, cell_start, order)
    _, _, n = sample_ref.emulate(rec, pos, h, mass, grid, cell_start, order)
    return u, n


def box_of(grid):
    lo = np.array([F(grid.gridMin[a]) for a in range(3)], F)
    hi = np.array([F(F(grid.gridMin[a]) + F(F(grid.dims[a]) * F(grid.cellSize))) for a in range(3)], F)
    return lo, hi


def advance(pool, u, n, cfg, gravity, box, dt):
    """(records after the advance, fate per record): fate 0 lives, 1 life, 2 age, 3 box, 4 non-finite."""
    dt = F(dt)
    g = np.asarray(gravity, F)
    x, v = pool["pos"].astype(F), pool["vel"].astype(F)
    spray = n < cfg.sprayBelow
    bubble = ~spray & (n > cfg.bubbleAbove)
    foam = ~spray & ~bubble
    with np.errstate(all="ignore"):
        vs = (v + (dt * g)[None, :].astype(F)).astype(F)
        dk = F(dt * F(cfg.kb))
        vb = ((v - (dk * g)[None, :].astype(F)).astype(F) + (F(cfg.kd) * (u - v).astype(F)).astype(F)).astype(F)
        vn = np.where(spray[:, None], vs, np.where(bubble[:, None], vb, u)).astype(F)
        xn = (x + (dt * vn).astype(F)).astype(F)
        life = np.where(foam, (pool["life"] - dt).astype(F), pool["life"]).astype(F)
        age = (pool["age"] + dt).astype(F)
    out = pool.copy()
    out["pos"], out["vel"], out["life"], out["age"] = xn, vn, life, age
    out["kind"] = np.where(spray, SPRAY, np.where(bubble, BUBBLE, FOAM)).astype(U32)
    lo, hi = box
    nonfin = ~np.isfinite(xn).all(axis=1)
    with np.errstate(invalid="ignore"):
        outside = ((xn < lo[None, :]) | (xn > hi[None, :])).any(axis=1)
        no_life = ~(life > 0)
        old = age > F(cfg.maxAge)
    fate = np.where(nonfin, 4, np.where(outside, 3, np.where(no_life, 1, np.where(old, 2, 0))))
    return out, fate


def children(rec, cfg, dt, c):
    """Children per fluid particle this substep (id = index)."""
    dt = F(dt)
    foam = rec["padA"].astype(F)
    rho = rec["density"].astype(F)
    with np.errstate(all="ignore"):
        inv = np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(F)
        ok = (rec["isGhost"] == 0) & (inv > 0) & np.isfinite(foam) & (foam > F(cfg.threshold))
        rd = F(F(cfg.rate) * dt)
        lam = (rd * (foam - F(cfg.threshold)).astype(F)).astype(F)
        f = np.floor((lam + uniform(cfg.seed, np.arange(len(rec)), c, 0)).astype(F))
        cnt = np.where(f < F(cfg.maxPerParent), np.maximum(f, 0), cfg.maxPerParent)
    return np.where(ok, np.nan_to_num(cnt, nan=float(cfg.maxPerParent)), 0).astype(np.int64)


def newborn(rec, cnt, cfg, h, c):
    """The newborn in (parent id, k) order."""
    parents = np.repeat(np.arange(len(rec)), cnt)
    first = np.cumsum(cnt) - cnt
    k = np.arange(len(parents)) - np.repeat(first, cnt)
    out = np.zeros(len(parents), DIFFUSE_DTYPE)
    sh = F(F(cfg.spread) * F(h))
    d0 = 1 + 4 * k
    for a in range(3):
        o = (F(2.0) * uniform(cfg.seed, parents, c, d0 + a) - F(1.0)).astype(F)
        out["pos"][:, a] = (rec["pos"][parents, a].astype(F) + (sh * o).astype(F)).astype(F)
    span = F(F(cfg.lifeMax) - F(cfg.lifeMin))
    out["life"] = (F(cfg.lifeMin) + (uniform(cfg.seed, parents, c, d0 + 3) * span).astype(F)).astype(F)
    out["vel"] = rec["vel"][parents, :3]
    out["parent"] = parents.astype(U32)
    out["birth"] = U32(int(c) & 0xFFFFFFFF)
    out["kind"] = FOAM
    return out


def step(pool, u, n, rec, cfg, h, gravity, grid, dt, c, totals=None):
    """One substep: (pool', totals').  totals: a dict from new_totals() / a previous call."""
    t = dict(totals or new_totals())
    t["aliveByKind"] = list(t["aliveByKind"])
    moved, fate = advance(pool, u, n, cfg, gravity, box_of(grid), dt)
    keep = moved[fate == 0]
    cnt = children(rec, cfg, dt, c)
    born = newborn(rec, cnt, cfg, h, c)
    room = int(cfg.capacity) - len(keep)
    dropped = max(len(born) - room, 0)
    born = born[:len(born) - dropped]
    out = np.concatenate([keep, born])
    t["substeps"] += 1
    t["spawned"] += int(cnt.sum())
    t["dropped"] += dropped
    for key, code in (("diedLife", 1), ("diedAge", 2), ("leftBox", 3), ("nonFinite", 4)):
        t[key] += int((fate == code).sum())
    t["alive"] = len(out)
    t["aliveByKind"] = [int((keep["kind"] == q).sum()) + (len(born) if q == FOAM else 0) for q in range(3)]
    return out, t


def step_on(oracle, rec, op, pool, cfg, dt, c, totals=None):
    b = oracle.build_grid(rec, op)
    u, n = sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
    return step(pool, u, n, rec, cfg, op.h, tuple(op.gravity), b["grid"], dt, c, totals)


# ---- the shared scene of tests/test_diffuse_cpu.py and tests/test_gpu_diffuse.py ----
SCENE_STEPS = 24
SCENE_CONFIG = dict(capacity=4096, seed=11, threshold=0.2, rate=3000.0, lifeMin=0.002, lifeMax=0.03, spread=0.5, maxAge=0.02,
                    sprayBelow=4, bubbleAbove=6, kb=2.0, kd=0.5, maxPerParent=3)
_cache = {}


def scene(pkg, oracle):
    """4096 particles in a 16^3 grid after one oracle substep (the records carry densities), foam painted on every 16th particle, a
    wave impulse on top, and four caller-made records: one about to leave the box, one non-finite, one short-lived, one plain.
    Returns (records, SphParams, OParams, pool0)."""
    from conftest import small_scene, to_oracle_params
    if "scene" not in _cache:
        rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
        op = to_oracle_params(oracle, sp)
        rec = oracle.substep(rec, op)
        rng = np.random.default_rng(14)
        rec["padA"][::16] = rng.random(len(rec[::16])).astype(F)
        rec = oracle.wave_impulse(rec, 40.0, 1.5, 0.25, (0.0, 1.0, 0.0))
        pool = np.zeros(4, DIFFUSE_DTYPE)
        pool["pos"] = [(2.2, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, 0.0, 0.0), (0.1, 1.9, 0.2)]
        pool["vel"] = [(100.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 5.0, 0.0)]
        pool["life"] = [1.0, 1.0, 0.0015, 1.0]
        pool["parent"] = 0xFFFFFFFF
        _cache["scene"] = (rec, sp, op, pool)
    rec, sp, op, pool = _cache["scene"]
    return rec.copy(), sp, op, pool.copy()


def scene_reference(pkg, oracle, capacity=None):
    """The scene run for SCENE_STEPS substeps by the restatement, once per capacity: a list of (pool, totals) after every substep."""
    key = ("run", capacity)
    if key not in _cache:
        rec, sp, op, pool = scene(pkg, oracle)
        cfg = pkg.diffuse_config(**dict(SCENE_CONFIG, **({} if capacity is None else {"capacity": capacity})))
        t = new_totals()
        t["seeded"] = len(pool)
        t["alive"] = len(pool)
        snaps = []
        for i in range(SCENE_STEPS):
            pool, t = step_on(oracle, rec, op, pool, cfg, F(op.timeStep), i, t)
            rec = oracle.substep(rec, op)
            snaps.append((pool.copy(), dict(t, aliveByKind=list(t["aliveByKind"]))))
        _cache[key] = snaps
    return _cache[key]
