"""Numpy restatement of the crest births of the diffuse pool (include/sph_abi.h "births at wave crests"), on the
SphShell rows that shell_host gives for the substep's entry state.

crest_children(): who qualifies and how many children the crest term alone gives.  step(): one substep of diffuse_ref.step with the
crest children behind the foam term's, and the crest books.  Every fp32 operation is rounded on its own; dot3 is the engine's
fmaf(az, bz, fmaf(ay, by, ax * bx)), restated by fma32(), which rounds the exact a * b + c once.
"""
from __future__ import annotations

import numpy as np

import diffuse_ref as D

F = np.float32
MEMBER, ISOLATED = 1, 2
DRAW = 33                                                                    # the first draw the eight children of a parent leave
BOOKS = ("acting", "crestSpawned", "shellSize")


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64; the float64 sum is rounded to odd (TwoSum gives the error), so
    that the final rounding to float32 is that of the exact value."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0)
        bits = np.atleast_1d(s).view(np.int64).copy()
        fx, ev, sv = np.atleast_1d(fix), np.atleast_1d(e), np.atleast_1d(s)
        away = (ev > 0) == (sv > 0)                                          # the exact sum lies further from zero than s
        bits = np.where(fx & ~away, bits - 1, bits)                          # the truncated sum ...
        bits = np.where(fx, bits | 1, bits)                                  # ... with the sticky bit
        return bits.view(np.float64).reshape(np.shape(s)).astype(F)


def dot3(a, b):
    """dot3 of sph_device.h over the rows of two (n, 3) float32 arrays."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(F)))


def window(x, lo, hi):
    """fminf(fmaxf((x - lo) / (hi - lo), 0), 1) in fp32."""
    with np.errstate(all="ignore"):
        q = ((np.asarray(x, F) - F(lo)).astype(F) / F(F(hi) - F(lo))).astype(F)
    return np.minimum(np.maximum(q, F(0.0)), F(1.0)).astype(F)


def acts(crest, c):
    return int(c) % int(crest.every) == 0


def potentials(rec, rows, crest):
    """(qualifies, pc, pk, speed, aligned) per particle (id = index)."""
    v = rec["vel"][:, :3].astype(F)
    rho = rec["density"].astype(F)
    with np.errstate(all="ignore"):
        inv = np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(F)
        sp2 = dot3(v, v)
        sp = np.sqrt(sp2).astype(F)
        along = dot3(v, rows["normal"].astype(F))
        aligned = along >= (F(crest.align) * sp).astype(F)
    member = (rows["flags"] & MEMBER) != 0
    isolated = (rows["flags"] & ISOLATED) != 0
    aligned = member & ~isolated & np.isfinite(sp2) & (sp > 0) & aligned     # shell members that move along their normal
    ok = (rec["isGhost"] == 0) & (inv > 0) & aligned
    return ok, window(rows["crest"], crest.crestMin, crest.crestMax), window(sp, crest.speedMin, crest.speedMax), sp, aligned


def crest_children(rec, rows, cfg, crest, dt, c):
    """Children of the crest term per particle on an acting substep, before the cap on the sum with the foam term's."""
    ok, pc, pk, _, _ = potentials(rec, rows, crest)
    with np.errstate(all="ignore"):
        p = (pc * pk).astype(F)
        rate = F(F(F(crest.rate) * F(dt)) * F(crest.every))
        lam = (rate * p).astype(F)
        f = np.floor((lam + D.uniform(cfg.seed, np.arange(len(rec)), c, DRAW)).astype(F))
        cnt = np.where(f < F(cfg.maxPerParent), np.maximum(f, 0), cfg.maxPerParent)
    return np.where(ok & (p > 0), np.nan_to_num(cnt, nan=float(cfg.maxPerParent)), 0).astype(np.int64)


def children(rec, rows, cfg, crest, dt, c):
    """(children per particle, those of them the foam term gave)."""
    foam = D.children(rec, cfg, dt, c)
    if crest is None or not acts(crest, c):
        return foam, foam
    return np.minimum(foam + crest_children(rec, rows, cfg, crest, dt, c), cfg.maxPerParent), foam


def step(pool, u, n, rec, rows, cfg, crest, h, gravity, grid, dt, c, totals=None):
    """diffuse_ref.step with the crest term: (pool', totals'); totals carries the crest books beside diffuse_ref's."""
    t = dict(totals or D.new_totals())
    for k in BOOKS:
        t.setdefault(k, 0)
    moved, fate = D.advance(pool, u, n, cfg, gravity, D.box_of(grid), dt)
    keep = moved[fate == 0]
    cnt, foam = children(rec, rows, cfg, crest, dt, c)
    born = D.newborn(rec, cnt, cfg, h, c)
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
    t["aliveByKind"] = [int((keep["kind"] == q).sum()) + (len(born) if q == D.FOAM else 0) for q in range(3)]
    if crest is not None and acts(crest, c):
        t["acting"] += 1
        t["crestSpawned"] += int((cnt - foam).sum())
        t["shellSize"] = int(((rows["flags"] & MEMBER) != 0).sum())
    return out, t


# ---- the settings of the shared scene (diffuse_ref.scene) in tests/test_diffuse_crest_cpu.py and tests/test_gpu_diffuse_crest.py ----
ROOMY = 65536                                                                # a capacity the scene never fills: dropped stays 0
SCENE_RADIUS = 1.5                                                           # in units of h
SCENE_CREST = dict(rate=4000.0, offset=0.10, minCount=0, flags=0, crestMin=0.25, crestMax=1.0, speedMin=10.0, speedMax=30.0, align=0.6, every=1)


def scene_crest(pkg, sp, **kw):
    return pkg.diffuse_crest_config(**{**SCENE_CREST, "radius": float(F(SCENE_RADIUS) * F(sp.param_h)), **kw})


def events(rec, rows, cfg, crest, dt, c):
    """What a substep on (rec, rows) contains, as a dict of counts: qualifiers, parents of the crest term alone (padA <= threshold),
    parents with children of both terms, and qualifiers whose pc / pk is clamped at 0 / at 1."""
    ok, pc, pk, _, aligned = potentials(rec, rows, crest)
    if not acts(crest, c):
        return {}
    cnt, foam = children(rec, rows, cfg, crest, dt, c)
    extra = cnt - foam
    with np.errstate(invalid="ignore"):
        low = ~(rec["padA"] > F(cfg.threshold))
    return dict(aligned=int(aligned.sum()), qualifiers=int(ok.sum()), crestBorn=int(extra.sum()), crestOnly=int(((extra > 0) & low).sum()),
                both=int(((extra > 0) & (foam > 0)).sum()), pc0=int((ok & (pc == 0)).sum()), pc1=int((ok & (pc == 1)).sum()),
                pk0=int((ok & (pk == 0)).sum()), pk1=int((ok & (pk == 1)).sum()))


_cache = {}


def scene_reference(pkg, oracle, capacity=None, every=1, n=None):
    """diffuse_ref.scene (its first n particles) run for SCENE_STEPS substeps by the restatement with the crest term on, once per
    setting: a list of (pool, totals, events) after every substep."""
    key = (capacity, every, n)
    if key not in _cache:
        rec, sp, op, pool = D.scene(pkg, oracle)
        rec = rec if n is None else rec[:n].copy()
        cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, **({} if capacity is None else {"capacity": capacity})))
        crest = scene_crest(pkg, sp, every=every)
        t = D.new_totals()
        t["seeded"] = t["alive"] = len(pool)
        snaps = []
        for i in range(D.SCENE_STEPS):
            rows = shell_rows(pkg, rec, sp, crest)
            b = oracle.build_grid(rec, op)
            u, cnt = D.sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
            ev = events(rec, rows, cfg, crest, F(op.timeStep), i)
            pool, t = step(pool, u, cnt, rec, rows, cfg, crest, op.h, tuple(op.gravity), b["grid"], F(op.timeStep), i, t)
            rec = oracle.substep(rec, op)
            snaps.append((pool.copy(), dict(t, aliveByKind=list(t["aliveByKind"])), ev))
        _cache[key] = snaps
    return _cache[key]


def shell_rows(pkg, rec, sp, crest):
    """The SphShell rows by id the crest term reads on the state rec: shell_host with the crest config's shell settings."""
    rows, _, _ = pkg.shell_host(rec, sp, radius=crest.radius if crest.radius > 0 else None, offset=crest.offset, min_count=crest.minCount,
                                fluid_only=bool(crest.flags & pkg.SPH_SHELL_FLUID_ONLY))
    return rows
