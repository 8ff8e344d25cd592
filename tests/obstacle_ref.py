"""Numpy restatement of the kinematic solid obstacles (include/sph_abi.h "obstacles").

fp32 with a correctly rounded fma (tracer_ref._fma) wherever the engine has one (dot3 only), every other fp32 operation rounded on its
own; the impulses in fp64.  A body is a dict of fp32 arrays (shape, size, c, q, M, v, w, res, fr).

bodies(arr, normalise): SphObstacle records -> bodies (the engine's set normalises the quaternion, the host functions do not).
apply(): one obstacle step on 80-byte records (index order, bodies 0..K-1 per particle); advance(): one pose advance.
step(): one substep of the engine with obstacles: oracle.substep (SPH pass + container), the obstacles, the pose advance, then the
fountain recycle of the oracle when one is given.
"""
from __future__ import annotations

import math

import numpy as np

import tracer_ref

F = np.float32
SPHERE, BOX, CAPSULE = 0, 1, 2
OBSTACLE_DTYPE = np.dtype([("shape", "<i4"), ("size", "<f4", (3,)), ("center", "<f4", (3,)), ("rotation", "<f4", (4,)),
                           ("vel", "<f4", (3,)), ("omega", "<f4", (3,)), ("restitution", "<f4"), ("friction", "<f4")])
_fma = tracer_ref._fma


def _dot3(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, (F(ax) * F(bx)) if np.ndim(ax) == 0 and np.ndim(bx) == 0 else (ax * bx).astype(F)))


def normalize(q):
    q = np.asarray(q, F)
    n2 = _fma(q[3], q[3], _fma(q[2], q[2], _fma(q[1], q[1], F(q[0] * q[0]))))
    ln = F(np.sqrt(F(n2[0] if np.ndim(n2) else n2)))
    return np.array([q[0] / ln, q[1] / ln, q[2] / ln, q[3] / ln], F)


def matrix(q):
    w, x, y, z = (F(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    one, two = F(1), F(2)
    return np.array([one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
                     two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
                     two * (xz - wy), two * (yz + wx), one - two * (xx + yy)], F)


def bodies(arr, normalise=True):
    out = []
    for o in np.asarray(arr, OBSTACLE_DTYPE):
        q = o["rotation"].astype(F)
        if normalise:
            q = normalize(q)
        out.append(dict(shape=int(o["shape"]), size=o["size"].astype(F).copy(), c=o["center"].astype(F).copy(), q=q, M=matrix(q),
                        v=o["vel"].astype(F).copy(), w=o["omega"].astype(F).copy(), res=F(o["restitution"]), fr=F(o["friction"])))
    return out


def to_array(bs):
    out = np.zeros(len(bs), OBSTACLE_DTYPE)
    for i, b in enumerate(bs):
        out[i]["shape"] = b["shape"]
        out[i]["size"] = b["size"]
        out[i]["center"] = b["c"]
        out[i]["rotation"] = b["q"]
        out[i]["vel"] = b["v"]
        out[i]["omega"] = b["w"]
        out[i]["restitution"] = b["res"]
        out[i]["friction"] = b["fr"]
    return out


def advance(bs, dt):
    """One substep of every pose: c += dt V; q = normalize(q + (0.5 dt) (0, omega) (x) q) and M rebuilt when omega != 0."""
    dt = F(dt)
    out = []
    for b in bs:
        b = dict(b, c=b["c"].copy(), q=b["q"].copy(), M=b["M"].copy())
        b["c"] = (b["c"] + (dt * b["v"]).astype(F)).astype(F)
        ox, oy, oz = (F(x) for x in b["w"])
        if not (ox == 0 and oy == 0 and oz == 0):
            w, x, y, z = (F(v) for v in b["q"])
            pw = -((ox * x + oy * y) + oz * z)
            px = (ox * w + oy * z) - oz * y
            py = (oy * w + oz * x) - ox * z
            pz = (oz * w + ox * y) - oy * x
            hd = F(F(0.5) * dt)
            b["q"] = normalize(np.array([w + hd * pw, x + hd * px, y + hd * py, z + hd * pz], F))
            b["M"] = matrix(b["q"])
        out.append(b)
    return out


def hit(b, mass, p, v, active):
    """One body against particles p, v ((n, 3) fp32) where `active`: (p', v', inside, took the u_n < 0 branch, terms (n, 6) fp64)."""
    c, M, sz = b["c"], b["M"], b["size"]
    n = len(p)
    with np.errstate(all="ignore"):
        d = [(p[:, a] - c[a]).astype(F) for a in range(3)]
        if b["shape"] == SPHERE:
            R = F(sz[0])
            r2 = _dot3(d[0], d[1], d[2], d[0], d[1], d[2])
            inside = active & (r2 < F(R * R))
            ln = np.sqrt(r2).astype(F)
            deg = ln == 0
            safe = np.where(deg, F(1), ln).astype(F)
            nrm = [np.where(deg, M[1 + 3 * a], (d[a] / safe).astype(F)).astype(F) for a in range(3)]
            q = [(c[a] + (R * nrm[a]).astype(F)).astype(F) for a in range(3)]
        else:
            l = [_dot3(d[0], d[1], d[2], np.full(n, M[j], F), np.full(n, M[3 + j], F), np.full(n, M[6 + j], F)) for j in range(3)]
            if b["shape"] == BOX:
                h = [F(sz[a]) for a in range(3)]
                al = [np.abs(l[a]) for a in range(3)]
                inside = active & (al[0] < h[0]) & (al[1] < h[1]) & (al[2] < h[2])
                gap = [(h[a] - al[a]).astype(F) for a in range(3)]
                cx = (gap[0] <= gap[1]) & (gap[0] <= gap[2])
                cy = ~cx & (gap[1] <= gap[2])
                cz = ~cx & ~cy
                pick = [cx, cy, cz]
                o, m = [], []
                for a in range(3):
                    s = np.where(l[a] >= 0, F(1), F(-1)).astype(F)
                    o.append(np.where(pick[a], (s * h[a]).astype(F), l[a]).astype(F))
                    m.append(np.where(pick[a], s, F(0)).astype(F))
            else:
                r, L = F(sz[0]), F(sz[1])
                sy = np.minimum(np.maximum(l[1], -L), L).astype(F)
                e = [l[0], (l[1] - sy).astype(F), l[2]]
                e2 = _dot3(e[0], e[1], e[2], e[0], e[1], e[2])
                inside = active & (e2 < F(r * r))
                ln = np.sqrt(e2).astype(F)
                deg = ln == 0
                safe = np.where(deg, F(1), ln).astype(F)
                m = [np.where(deg, F(1) if a == 0 else F(0), (e[a] / safe).astype(F)).astype(F) for a in range(3)]
                o = [(r * m[0]).astype(F), (sy + (r * m[1]).astype(F)).astype(F), (r * m[2]).astype(F)]
            row = [[np.full(n, M[3 * i + j], F) for j in range(3)] for i in range(3)]
            nrm = [_dot3(row[i][0], row[i][1], row[i][2], m[0], m[1], m[2]) for i in range(3)]
            q = [(c[i] + _dot3(row[i][0], row[i][1], row[i][2], o[0], o[1], o[2])).astype(F) for i in range(3)]
        rr = [(q[a] - c[a]).astype(F) for a in range(3)]
        w, V = b["w"], b["v"]
        s = [(V[0] + ((w[1] * rr[2]).astype(F) - (w[2] * rr[1]).astype(F)).astype(F)).astype(F),
             (V[1] + ((w[2] * rr[0]).astype(F) - (w[0] * rr[2]).astype(F)).astype(F)).astype(F),
             (V[2] + ((w[0] * rr[1]).astype(F) - (w[1] * rr[0]).astype(F)).astype(F)).astype(F)]
        u = [(v[:, a] - s[a]).astype(F) for a in range(3)]
        un = _dot3(u[0], u[1], u[2], nrm[0], nrm[1], nrm[2])
        neg = inside & (un < 0)
        aa = (F(-b["res"]) * un).astype(F)
        omf = F(F(1) - b["fr"])
        nv = []
        for a in range(3):
            t = (u[a] - (un * nrm[a]).astype(F)).astype(F)
            nv.append(((s[a] + (aa * nrm[a]).astype(F)).astype(F) + (omf * t).astype(F)).astype(F))
    p2, v2 = p.copy(), v.copy()
    for a in range(3):
        p2[:, a] = np.where(inside, q[a], p[:, a])
        v2[:, a] = np.where(neg, nv[a], v[:, a])
    m64 = np.float64(F(mass))
    J = np.zeros((n, 6), np.float64)
    for a in range(3):
        J[:, a] = np.where(neg, m64 * (v[:, a].astype(np.float64) - v2[:, a].astype(np.float64)), 0.0)
    R64 = [np.asarray(x, np.float64) for x in rr]
    J[:, 3] = np.where(neg, R64[1] * J[:, 2] - R64[2] * J[:, 1], 0.0)
    J[:, 4] = np.where(neg, R64[2] * J[:, 0] - R64[0] * J[:, 2], 0.0)
    J[:, 5] = np.where(neg, R64[0] * J[:, 1] - R64[1] * J[:, 0], 0.0)
    return p2, v2, inside, neg, J


def apply(bs, mass, rec):
    """One obstacle step on 80-byte records: (records, impulses (K, 6) correctly rounded sums, info).  info per body: touched count,
    u_n < 0 count, sum of |term| per component (K, 6), and the terms themselves."""
    rec = rec.copy()
    p = rec["pos"][:, :3].astype(F).copy()
    v = rec["vel"][:, :3].astype(F).copy()
    active = (rec["isGhost"] == 0) & np.isfinite(p).all(axis=1)
    imp = np.zeros((len(bs), 6), np.float64)
    info = dict(touched=np.zeros(len(bs), np.int64), negative=np.zeros(len(bs), np.int64), abs_sum=np.zeros((len(bs), 6)), terms=[])
    for k, b in enumerate(bs):
        p, v, inside, neg, J = hit(b, mass, p, v, active)
        info["touched"][k] = int(inside.sum())
        info["negative"][k] = int(neg.sum())
        info["abs_sum"][k] = np.abs(J).sum(axis=0)
        info["terms"].append(J[inside])
        for a in range(6):
            imp[k, a] = math.fsum(J[inside, a])
    rec["pos"][:, :3] = p
    rec["vel"][:, :3] = v
    return rec, imp, info


def impulse_bound(info):
    """2 (n_terms - 1) 2^-53 sum |t_i| per body and component: the worst case between two fp64 sums of the same terms in different orders."""
    n = np.maximum(info["touched"] - 1, 0).astype(np.float64)
    return 2.0 * n[:, None] * 2.0 ** -53 * info["abs_sum"]


def step(oracle, rec, op, bs, dt=None, fountain=None):
    """One engine substep with obstacles: (records, bodies, impulses, info)."""
    step_dt = F(op.timeStep if dt is None or dt <= 0 else dt)
    rec = oracle.substep(rec, op, dt=float(step_dt) if dt is not None and dt > 0 else -1.0)
    rec, imp, info = apply(bs, F(op.mass), rec)
    bs = advance(bs, step_dt)
    if fountain is not None and fountain.mode:
        rec = oracle.fountain_recycle(rec, op, fountain, float(step_dt), int(fountain.seed))
        fountain.seed = (int(fountain.seed) + 1) & 0xFFFFFFFF
    return rec, bs, imp, info
