"""Numpy references of the field sampler (include/sph_abi.h "field sampling").

emulate(): the sampler's own fp32 arithmetic over the candidates of oracle.build_grid's cells, in the canonical order (9 rows in
(dz, dy) order, members ascending by id): density / fraction / count as the kernel forms them.  fma is emulated through float64
(oracle._fma), which differs from a true fma in ~2^-29 of the cases.
brute(): float64 brute force over ALL particles within h (cellSize = h, so these are exactly the candidates that can count).
"""
from __future__ import annotations

import numpy as np

F = np.float32


def simk_consts(h: float, mass: float):
    """make_simk's h2 and mp6 in fp32 (csrc/sph_host.h)."""
    h = F(h)
    h2 = F(h * h)
    h3 = F(h2 * h)
    h6 = F(h3 * h3)
    h9 = F(h6 * h3)
    pi_f = F(3.141592653589)
    poly6 = F(F(315.0) / F(F(F(64.0) * pi_f) * h9))
    return h2, F(F(mass) * poly6)


def cell_of(points, g):
    """BuildGrid's cell formula in fp32: (x - gridMin) / cellSize, floorf, clamped; points must be finite."""
    out = []
    for a in range(3):
        q = (points[:, a].astype(F) - F(g.gridMin[a])) / F(g.cellSize)
        out.append(np.clip(np.floor(q), 0, g.dims[a] - 1).astype(np.int64))
    return out


def candidates(points, grid, cell_start, order):
    """(m, K) particle indices (or -1) of every probe's candidates in canonical order."""
    cx, cy, cz = cell_of(points, grid)
    gx, gy, gz = grid.dims[0], grid.dims[1], grid.dims[2]
    cs = np.asarray(cell_start, np.int64)
    parts = []
    xlo, xhi = np.maximum(cx - 1, 0), np.minimum(cx + 1, gx - 1)
    for r in range(9):
        nz, ny = cz + r // 3 - 1, cy + r % 3 - 1
        ok = (nz >= 0) & (nz < gz) & (ny >= 0) & (ny < gy)
        base = (np.clip(nz, 0, gz - 1) * gy + np.clip(ny, 0, gy - 1)) * gx
        qs = np.where(ok, cs[base + xlo], 0)
        qe = np.where(ok, cs[base + xhi + 1], 0)
        parts.append((qs, qe))
    width = max(int((qe - qs).max(initial=0)) for qs, qe in parts)
    cols = []
    for qs, qe in parts:
        j = np.arange(width)[None, :]
        slot = qs[:, None] + j
        cols.append(np.where(slot < qe[:, None], np.asarray(order, np.int64)[np.minimum(slot, max(len(order) - 1, 0))] if len(order) else -1, -1))
    return np.concatenate(cols, axis=1) if cols else np.zeros((len(points), 0), np.int64)


def emulate(rec, points, h, mass, grid, cell_start, order):
    """density, fraction and count as the sampler forms them (fp32, canonical order); non-finite probes -> 0."""
    from oracle.oracle import _dot3, _fma
    pts = np.asarray(points, F)[:, :3]
    fin = np.isfinite(pts).all(axis=1)
    safe = np.where(fin[:, None], pts, F(0))
    idx = candidates(safe, grid, cell_start, order)
    h2, mp6 = simk_consts(h, mass)
    pos = rec["pos"][:, :3].astype(F)
    rho = rec["density"].astype(F)
    inv = np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(F)
    m = len(pts)
    dsum = np.zeros(m, F)
    wsum = np.zeros(m, F)
    cnt = np.zeros(m, np.uint32)
    for k in range(idx.shape[1]):
        j = idx[:, k]
        ok = j >= 0
        jj = np.where(ok, j, 0)
        d = (safe - pos[jj]).astype(F)
        r2 = _dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
        t = np.maximum(F(h2) - r2, F(0)).astype(F)
        dsum = np.where(ok, _fma(F(1) * (t * t).astype(F), t, dsum), dsum)
        w = (((t * t).astype(F) * t).astype(F) * inv[jj]).astype(F)
        wsum = np.where(ok, (wsum + w).astype(F), wsum)
        cnt += (ok & (r2 < h2)).astype(np.uint32)
    dens = np.where(fin, (mp6 * dsum).astype(F), F(0))
    frac = np.where(fin, (mp6 * wsum).astype(F), F(0))
    return dens, frac, np.where(fin, cnt, 0).astype(np.uint32)


def brute(rec, points, h, mass, chunk=512):
    """float64 fields over all particles within h.  Returns a dict with density, fraction, pressure, vel (m, 3), count, and
    `edge`: pairs with |r^2 - h^2| <= 1e-5 h^2 (count may legitimately differ by those)."""
    h = float(h)
    h2 = h * h
    mp6 = float(mass) * 315.0 / (64.0 * np.pi * h ** 9)
    pos = rec["pos"][:, :3].astype(np.float64)
    rho = rec["density"].astype(F)
    inv = np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(np.float64)
    vel = rec["vel"][:, :3].astype(np.float64)
    prs = rec["pressure"].astype(np.float64)
    pts = np.asarray(points, np.float64)[:, :3]
    m = len(pts)
    out = dict(density=np.zeros(m), fraction=np.zeros(m), pressure=np.zeros(m), vel=np.zeros((m, 3)), count=np.zeros(m, np.int64),
               edge=np.zeros(m, np.int64), wsum=np.zeros(m))
    fin = np.isfinite(pts).all(axis=1)
    for a in range(0, m, chunk):
        b = min(a + chunk, m)
        p = np.where(fin[a:b, None], pts[a:b], 1e30)
        d2 = ((p[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
        t = np.maximum(h2 - d2, 0.0)
        t3 = t ** 3
        w = t3 * inv[None, :]
        ws = w.sum(axis=1)
        out["density"][a:b] = mp6 * t3.sum(axis=1)
        out["fraction"][a:b] = mp6 * ws
        out["wsum"][a:b] = ws
        nz = ws > 0
        safe = np.where(nz, ws, 1.0)
        out["vel"][a:b] = np.where(nz[:, None], (w @ vel) / safe[:, None], 0.0)
        out["pressure"][a:b] = np.where(nz, (w @ prs) / safe, 0.0)
        out["count"][a:b] = (d2 < h2).sum(axis=1)
        out["edge"][a:b] = (np.abs(d2 - h2) <= 1e-5 * h2).sum(axis=1)
    for k in ("density", "fraction", "pressure", "count", "edge", "wsum"):
        out[k][~fin] = 0
    out["vel"][~fin] = 0
    return out


def gauge_columns(frac_fn, cols, y_lo, y_hi, dy):
    """Heights of a water_level column (descending from y_hi) and the (c, k) probe points."""
    ys = F(y_hi) - np.arange(int(np.floor((y_hi - y_lo) / dy + 1e-6)) + 1, dtype=F) * F(dy)
    pts = np.zeros((len(cols), len(ys), 3), F)
    pts[:, :, 0] = np.asarray(cols, F)[:, None, 0]
    pts[:, :, 1] = ys[None, :]
    pts[:, :, 2] = np.asarray(cols, F)[:, None, 1]
    return ys, pts
