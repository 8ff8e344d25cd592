"""numpy restatements of the diffusing scalar channels, written from DESIGN.md section 3h / include/sph_abi.h (not from the kernels).

step32(): the substep's scalar update in fp32 with the operation order of section 3h, over the candidates of oracle.build_grid's
cells in canonical order (tests/sample_ref.candidates).  fma32 is a correctly rounded fp32 fma, so the result is meant to be
bit-equal to sph_scalars_step_host.
step64(): the same formula evaluated in float64 on the same (fp32) inputs: the reference of the conservation, maximum-principle
and consistency checks, and the source of their rounding bound.
"""
from __future__ import annotations

import numpy as np

import sample_ref

F = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c) of float32 arrays: the product is exact in float64; the float64 sum is moved off a
    float32 rounding tie in the direction of its own rounding error (TwoSum) before it is rounded to float32."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        tie = np.isfinite(s) & ((np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0)
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def dot3(ax, ay, az, bx, by, bz):
    return fma32(az, bz, fma32(ay, by, (ax * bx).astype(F)))


def klap(mass, h):
    """(float)((90 m) / (pi ((h^2 h^2) h^2))) in double, m and h being the fp32 members."""
    hd = float(F(h))
    h2 = hd * hd
    return F((90.0 * float(F(mass))) / (3.14159265358979323846 * ((h2 * h2) * h2)))


def inv_rho(rec):
    rho = rec["density"].astype(F)
    return np.where(rho > 0, F(1.0) / np.where(rho > 0, rho, F(1)), F(0)).astype(F)


def targets(rec):
    """Records that are updated: isGhost == 0, finite position, 1/rho > 0."""
    return (rec["isGhost"] == 0) & np.isfinite(rec["pos"][:, :3]).all(axis=1) & (inv_rho(rec) > 0)


def _coeffs(K, diffusivity, decay):
    return (np.broadcast_to(np.asarray(diffusivity, F), (K,)).astype(F), np.broadcast_to(np.asarray(decay, F), (K,)).astype(F))


def _candidates(rec, grid, cell_start, order):
    pos = rec["pos"][:, :3].astype(F)
    fin = np.isfinite(pos).all(axis=1)
    safe = np.where(fin[:, None], pos, F(0))
    return sample_ref.candidates(safe, grid, cell_start, order)


def step32(rec, values, h, mass, diffusivity, decay, dt, grid, cell_start, order):
    """((n, K) float32 values one substep later, the diffusion number as float32) in the engine's fp32 arithmetic."""
    c = np.ascontiguousarray(values, F).reshape(len(rec), -1)
    n, K = c.shape
    D, lam = _coeffs(K, diffusivity, decay)
    h, dt = F(h), F(dt)
    h2 = F(h * h)
    soft = F(F(0.01) * h2)
    pos = rec["pos"][:, :3].astype(F)
    inv = inv_rho(rec)
    ghost = rec["isGhost"] != 0
    tgt = targets(rec)
    idx = _candidates(rec, grid, cell_start, order)
    me = np.arange(n)
    a = np.zeros((n, K), F)
    W = np.zeros(n, F)
    with np.errstate(all="ignore"):
        for col in range(idx.shape[1]):
            j = idx[:, col]
            ok = (j >= 0) & (j != me)
            jj = np.where(ok, j, 0)
            d = (pos - pos[jj]).astype(F)
            r2 = dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
            part = ok & tgt & (r2 > 0) & (r2 < h2) & (inv[jj] > 0) & ~ghost[jj]
            r = np.sqrt(r2).astype(F)
            u = (h - r).astype(F)
            G = (((u * u).astype(F) * r).astype(F) / (r2 + soft).astype(F)).astype(F)
            w = ((inv * inv[jj]).astype(F) * G).astype(F)
            for k in range(K):
                a[:, k] = np.where(part, fma32(w, (c[jj, k] - c[:, k]).astype(F), a[:, k]), a[:, k])
            W = np.where(part, (W + w).astype(F), W)
        kl = klap(mass, h)
        out = c.copy()
        for k in range(K):
            dk = F(D[k] * kl)
            new = (c[:, k] + (dt * ((dk * a[:, k]).astype(F) - (lam[k] * c[:, k]).astype(F)).astype(F)).astype(F)).astype(F)
            out[:, k] = np.where(tgt, new, c[:, k])
        s = (F(dt * F(D.max() * kl)) * W).astype(F)
    bits = s[tgt].view(np.uint32)
    return out, (np.array([bits.max()], np.uint32).view(F)[0] if len(bits) else F(0))


def step64(rec, values, h, mass, diffusivity, decay, dt, grid, cell_start, order):
    """The same formula in float64 on the same inputs (fp32 positions, densities, values, members).  Returns a dict:
    values (n, K) float64 one substep later, number (n,) s_i, pairs (n,) participating pairs, spread (n, K) sum_j w |c_j - c_i|,
    spread_hi the same with (h - r)^2 replaced by h^2 in w (an upper bound of w that does not cancel), W (n,) sum_j w."""
    c = np.asarray(values, np.float64).reshape(len(rec), -1)           # (fp32 values pass unchanged; a float64 run carries its own)
    n, K = c.shape
    D, lam = _coeffs(K, diffusivity, decay)
    D, lam = D.astype(np.float64), lam.astype(np.float64)
    h, dt = float(F(h)), float(F(dt))
    h2 = h * h
    pos = rec["pos"][:, :3].astype(np.float64)
    inv = inv_rho(rec).astype(np.float64)
    ghost = rec["isGhost"] != 0
    tgt = targets(rec)
    idx = _candidates(rec, grid, cell_start, order)
    me = np.arange(n)
    a = np.zeros((n, K))
    spread = np.zeros((n, K))
    spread_hi = np.zeros((n, K))
    W = np.zeros(n)
    pairs = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for col in range(idx.shape[1]):
            j = idx[:, col]
            ok = (j >= 0) & (j != me)
            jj = np.where(ok, j, 0)
            d = pos - pos[jj]
            r2 = (d * d).sum(axis=1)
            part = ok & tgt & (r2 > 0) & (r2 < h2) & (inv[jj] > 0) & ~ghost[jj]
            r = np.sqrt(r2)
            w = np.where(part, (inv * inv[jj]) * ((h - r) ** 2 * r) / (r2 + 0.01 * h2), 0.0)
            a += w[:, None] * (c[jj] - c)
            spread += w[:, None] * np.abs(c[jj] - c)
            spread_hi += np.where(part, (inv * inv[jj]) * (h2 * r) / (r2 + 0.01 * h2), 0.0)[:, None] * np.abs(c[jj] - c)
            W += w
            pairs += part
    kl = float(klap(mass, h))
    new = c + dt * (D[None, :] * kl * a - lam[None, :] * c)
    return dict(values=np.where(tgt[:, None], new, c), number=dt * D.max() * kl * W, pairs=pairs, spread=spread, spread_hi=spread_hi, W=W,
                targets=tgt, scale=dt * D[None, :] * kl)


def rounding_bound(ref, values):
    """Per particle and channel, the forward-error bound of the particle's fma chain and finish:
    (pairs_i + 4) eps32 (|c_i| + dt D kLap sum_j w |c_j - c_i|), from the float64 evaluation `ref` = step64(...).  The weights w are
    bitwise symmetric in the engine, so their own rounding cancels in a sum over the particles; what does not cancel is one rounding
    per fma of the chain (each at most eps32 times the running sum, itself at most the spread) and the four operations of the finish."""
    c = np.abs(np.asarray(values, np.float64).reshape(len(ref["pairs"]), -1))
    b = (ref["pairs"][:, None] + 4.0) * EPS32 * (c + ref["scale"] * ref["spread"])
    return np.where(ref["targets"][:, None], b, 0.0)


def value_bound(ref, values):
    """Bound of |fp32 value - float64 value| after one substep: rounding_bound plus the rounding of the weights themselves, which
    does not cancel here.  A weight is formed by 3 subtractions, 3 operations of the dot product, a square root, h - r, 3 products,
    an addition, a division and 2 more products: 16 roundings, each at most eps32 of a quantity bounded by the weight with
    (h - r)^2 replaced by h^2 (the subtraction h - r cancels, its absolute error does not grow)."""
    return rounding_bound(ref, values) + np.where(ref["targets"][:, None], 16.0 * EPS32 * ref["scale"] * ref["spread_hi"], 0.0)


def cubic_lattice(pkg, oracle, m, spacing_over_h, h=0.28, rho0=1000.0):
    """m^3 particles on a cubic lattice of the given spacing with mass rho0 a^3, in a box that holds them with room to spare (no
    periodic images: the outer particles see less than full support).  The records carry the density the engine's own density sweep
    gives this lattice, max(mp6 sum (h2 - r2)^3, rho0 / 2) in its fp32 arithmetic (sample_ref.emulate, which test_sample_cpu pins to
    the pass density bit for bit): that is what every record of an engine holds after a substep, never m / a^3.  Returns
    (records, params)."""
    from conftest import to_oracle_params
    a = F(spacing_over_h) * F(h)
    g = (np.arange(m, dtype=F) - F(m - 1) / F(2)) * a
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)
    rec = np.zeros(len(pos), pkg.PARTICLE_DTYPE)
    rec["pos"][:, :3] = pos
    rec["pos"][:, 3] = 1.0
    rec["isActive"] = 1
    half = float(a) * m / 2 + 2 * h
    sp = pkg.default_params(param_h=h, param_mass=float(rho0 * float(a) ** 3), param_restDensity=rho0, param_boxHalf=(half, half, half),
                            param_boxCenter=(0.0, 0.0, 0.0), param_boxEulerDeg=(0.0, 0.0, 0.0), grid_cap=400)
    b = oracle.build_grid(rec, to_oracle_params(oracle, sp))
    dens, _, _ = sample_ref.emulate(rec, rec["pos"], sp.param_h, sp.param_mass, b["grid"], b["cell_start"], b["order"])
    rec["density"] = np.maximum(dens, F(0.5) * F(rho0))
    return rec, sp


def paint(rec, values, center, radius, channel, value, mode):
    """sph_scalars_paint: channel = value (mode 0, SPH_SCALAR_SET) or channel += value (mode 1, one fp32 add) for every record with
    isGhost == 0 whose position lies strictly inside the sphere, fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < radius * radius with d = x - center
    (a non-finite coordinate is never inside).  A new (n, K) array."""
    c = np.ascontiguousarray(values, F).reshape(len(rec), -1).copy()
    pos = rec["pos"][:, :3].astype(F)
    ce = np.asarray(center, F)
    with np.errstate(all="ignore"):
        d = [(pos[:, a] - ce[a]).astype(F) for a in range(3)]
        inside = (rec["isGhost"] == 0) & (dot3(d[0], d[1], d[2], d[0], d[1], d[2]) < F(F(radius) * F(radius)))
        new = np.full(len(rec), F(value), F) if mode == 0 else (c[:, channel] + F(value)).astype(F)
    c[:, channel] = np.where(inside, new, c[:, channel])
    return c


def moments(values, tgt, particle_cell):
    """Per channel over the targets with a finite value, as sph_scalars_moments forms them: count, the statistics' fixed-order fp64
    sum and sum of squares (slots in canonical order, +0.0 outside the set), (min, id), (max, id)."""
    import stats_ref
    v = np.ascontiguousarray(values, F).reshape(len(tgt), -1)
    ids = np.arange(len(tgt), dtype=np.int64)
    order = np.lexsort((ids, np.asarray(particle_cell, np.int64)))
    out = []
    for k in range(v.shape[1]):
        inset = tgt & np.isfinite(v[:, k])
        x = np.where(inset, v[:, k].astype(np.float64), 0.0)
        out.append(dict(count=int(inset.sum()), sum=stats_ref.tree_sum(x[order]), sum_squares=stats_ref.tree_sum((x * x)[order]),
                        min=stats_ref._extreme(v[inset, k], ids[inset], True), max=stats_ref._extreme(v[inset, k], ids[inset], False)))
    return out


def shepard32(rec, values, channel, points, h, grid, cell_start, order):
    """Shepard value sum w_j c_j / sum w_j of a channel at the points, in the sampler's fp32 arithmetic and order (ghost records
    included, as the sampler includes them); 0 where sum w_j = 0 and for non-finite points."""
    c = np.ascontiguousarray(values, F).reshape(len(rec), -1)[:, channel]
    pts = np.asarray(points, F)[:, :3]
    fin = np.isfinite(pts).all(axis=1)
    safe = np.where(fin[:, None], pts, F(0))
    idx = sample_ref.candidates(safe, grid, cell_start, order)
    h2 = F(F(h) * F(h))
    pos = rec["pos"][:, :3].astype(F)
    inv = inv_rho(rec)
    num = np.zeros(len(pts), F)
    wsum = np.zeros(len(pts), F)
    with np.errstate(all="ignore"):
        for col in range(idx.shape[1]):
            j = idx[:, col]
            ok = j >= 0
            jj = np.where(ok, j, 0)
            d = (safe - pos[jj]).astype(F)
            t = np.maximum(h2 - dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]), F(0)).astype(F)
            t = np.where(np.isnan(t), F(0), t)                       # fmaxf(NaN, 0) = 0
            w = (((t * t).astype(F) * t).astype(F) * inv[jj]).astype(F)
            wsum = np.where(ok, (wsum + w).astype(F), wsum)
            num = np.where(ok, fma32(w, c[jj], num), num)
        out = np.where(wsum > 0, (num / np.where(wsum > 0, wsum, F(1))).astype(F), F(0))
    return np.where(fin, out, F(0)).astype(F)
