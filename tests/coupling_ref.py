"""Numpy restatement of the active scalars (include/sph_abi.h "active scalars"): continuous sources and the
buoyancy kick on the output state of a substep, written from the contract (not from the kernel).

fp32 with scalar_ref.fma32 / dot3 wherever section 3i has an fma (the frame change, the sphere test, the buoyancy sum), every other
operation rounded on its own.  A source is a record of SOURCE_DTYPE; bodies are obstacle_ref bodies (dicts with c and M).
couple(): the step on 80-byte records in index order: (records, values, books) with the books summed by math.fsum.
books_bound(): 2 (n - 1) 2^-53 sum |term| per source, the worst case between two fp64 sums of the same terms in different orders.
"""
from __future__ import annotations

import math

import numpy as np

from scalar_ref import dot3, fma32

F = np.float32
SPHERE, BOX = 0, 1
RATE, RELAX = 0, 1
SOURCE_DTYPE = np.dtype([("shape", "<i4"), ("channel", "<i4"), ("mode", "<i4"), ("body", "<i4"), ("center", "<f4", (3,)), ("size", "<f4", (3,)),
                         ("rate", "<f4"), ("target", "<f4"), ("pad", "<f4", (4,))])
assert SOURCE_DTYPE.itemsize == 64


def source(shape, center, size, channel=0, mode=RATE, rate=0.0, target=0.0, body=-1):
    s = np.zeros(1, SOURCE_DTYPE)[0]
    s["shape"], s["channel"], s["mode"], s["body"] = shape, channel, mode, body
    s["center"] = center
    s["size"] = size
    s["rate"], s["target"] = rate, target
    return s


def targets(rec):
    """Records the step acts on: isGhost == 0 and a finite position."""
    return (rec["isGhost"] == 0) & np.isfinite(rec["pos"][:, :3]).all(axis=1)


def inside(src, bodies, pos):
    """Strictly inside the source's region, per particle ((n, 3) fp32 positions; a non-finite coordinate is never inside)."""
    n = len(pos)
    p = [pos[:, a].astype(F) for a in range(3)]
    ce = src["center"].astype(F)
    sz = src["size"].astype(F)
    with np.errstate(all="ignore"):
        if int(src["body"]) >= 0:
            b = bodies[int(src["body"])]
            c, M = b["c"], b["M"]
            q = [(p[a] - c[a]).astype(F) for a in range(3)]
            col = lambda j: [np.full(n, M[j], F), np.full(n, M[3 + j], F), np.full(n, M[6 + j], F)]
            d = [(dot3(q[0], q[1], q[2], *col(j)) - ce[j]).astype(F) for j in range(3)]
        else:
            d = [(p[a] - ce[a]).astype(F) for a in range(3)]
        if int(src["shape"]) == SPHERE:
            return dot3(d[0], d[1], d[2], d[0], d[1], d[2]) < F(sz[0] * sz[0])
        return (np.abs(d[0]) < sz[0]) & (np.abs(d[1]) < sz[1]) & (np.abs(d[2]) < sz[2])


def apply_source(src, dt, c):
    """c' of a hit: a multiply and then an add; RELAX clamped into the closed interval between c and the target."""
    dt = F(dt)
    with np.errstate(all="ignore"):
        if int(src["mode"]) == RATE:
            return (c + F(dt * F(src["rate"]))).astype(F)
        a = F(min(F(dt * F(src["rate"])), F(1.0)))
        t = F(src["target"])
        r = (c + (a * (t - c).astype(F)).astype(F)).astype(F)
        return np.fmin(np.fmax(r, np.fmin(c, t)), np.fmax(c, t)).astype(F)     # (fminf / fmaxf: a NaN operand is ignored)


def kick(beta, ref, values, dt, g, vel):
    """((n, 3) velocities after the kick, the mask of the records written)."""
    c = np.ascontiguousarray(values, F)
    n, K = c.shape
    dt = F(dt)
    with np.errstate(all="ignore"):
        s = np.zeros(n, F)
        for k in range(K):
            s = fma32(np.full(n, F(beta[k]), F), (c[:, k] - F(ref[k])).astype(F), s)
        on = np.isfinite(s) & (s != 0)
        f = (dt * s).astype(F)
        out = vel.copy()
        for a in range(3):
            out[:, a] = np.where(on, (vel[:, a] - (f * F(g[a])).astype(F)).astype(F), vel[:, a])
    return out, on


def couple(rec, values, dt, gravity, beta=None, ref=None, sources=(), bodies=()):
    """The coupling step of one substep on 80-byte records: (records, (n, K) values, books).  books: sums (correctly rounded, math.fsum),
    hits, abs_sum (sum |term|) per source and the terms themselves."""
    rec = rec.copy()
    c = np.ascontiguousarray(values, F).copy()
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    K = c.shape[1]
    tgt = targets(rec)
    pos = rec["pos"][:, :3].astype(F)
    S = len(sources)
    books = dict(sums=np.zeros(S), hits=np.zeros(S, np.uint64), abs_sum=np.zeros(S), terms=[])
    for i, src in enumerate(sources):
        ch = int(src["channel"])
        old = c[:, ch].copy()
        hit = tgt & inside(src, bodies, pos) & np.isfinite(old)
        new = apply_source(src, dt, old)
        c[:, ch] = np.where(hit, new, old)
        with np.errstate(all="ignore"):
            t = (new.astype(np.float64) - old.astype(np.float64))[hit]
        books["sums"][i] = math.fsum(t)
        books["hits"][i] = int(hit.sum())
        books["abs_sum"][i] = math.fsum(np.abs(t))
        books["terms"].append(t)
    if beta is not None:
        b = np.broadcast_to(np.asarray(beta, F), (K,))
        r = np.broadcast_to(np.asarray(0.0 if ref is None else ref, F), (K,))
        v = rec["vel"][:, :3].astype(F)
        out, on = kick(b, r, c, dt, gravity, v)
        rec["vel"][:, :3] = np.where((tgt & on)[:, None], out, v)
    return rec, c, books


def books_bound(hits, abs_sum):
    """2 (n - 1) 2^-53 sum |t_i| per source: any two fp64 sums of the same n terms, in whatever order, differ by no more (each is within
    (n - 1) 2^-53 sum |t_i| of the exact sum, to first order; the factor 2 also covers a comparison against the correctly rounded sum)."""
    n = np.maximum(np.asarray(hits, np.float64) - 1.0, 0.0)
    return 2.0 * n * 2.0 ** -53 * np.asarray(abs_sum, np.float64)
