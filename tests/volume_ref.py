"""Numpy restatement of the signed distance lattices (include/sph_abi.h "signed distance lattices").

fp32 with a correctly rounded fma wherever the engine has one (dot3 only), every other fp32 operation rounded on its own; the impulses
and the winding number in fp64.  A volume is a dict (values (nz, ny, nx) fp32, dims (nx, ny, nz), spacing, half, inv).

volume(values, spacing): the dict.  sample(): trilinear phi and gradient.  project(): the two-step projection of section 3f.
apply(): one obstacle step of section 3e with bodies bound to volumes (bindings[b] = index into vols or -1).  step(): one engine substep.
mesh_distance(): min over triangles of the squared distance to the closest point (region walk), sign from the winding number in fp64.
"""
from __future__ import annotations

import math

import numpy as np

import obstacle_ref as R

F = np.float32
_fma = R._fma
_dot3 = R._dot3


def volume(values, spacing):
    v = np.ascontiguousarray(values, F)
    nz, ny, nx = v.shape
    sp = np.broadcast_to(np.asarray(spacing, F), (3,)).astype(F)
    dims = (nx, ny, nz)
    half = np.array([F(F(0.5) * F(dims[a] - 1)) * sp[a] for a in range(3)], F)
    inv = np.array([F(1) / sp[a] for a in range(3)], F)
    return dict(values=v, dims=dims, spacing=sp, half=half, inv=inv)


def _lerp(a, b, f):
    return (a + (f * (b - a).astype(F)).astype(F)).astype(F)


def sample(vol, l, clamp=False):
    """phi, gradient (n, 3) (divided by the spacing, not normalised) and `within` at local points l (n, 3) fp32."""
    l = np.asarray(l, F).reshape(-1, 3)
    v, dims = vol["values"], vol["dims"]
    with np.errstate(all="ignore"):
        g = [((l[:, a] + vol["half"][a]).astype(F) * vol["inv"][a]).astype(F) for a in range(3)]
        top = [F(dims[a] - 1) for a in range(3)]
        if clamp:
            g = [np.fmin(np.fmax(g[a], F(0)), top[a]).astype(F) for a in range(3)]
            within = np.ones(len(l), bool)
        else:
            within = np.ones(len(l), bool)
            for a in range(3):
                within &= (g[a] >= 0) & (g[a] <= top[a])
        gs = [np.where(within, g[a], F(0)).astype(F) for a in range(3)]
        i = [np.minimum(np.floor(gs[a]).astype(np.int64), dims[a] - 2) for a in range(3)]
        f = [(gs[a] - i[a].astype(F)).astype(F) for a in range(3)]
        c = {}
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c[dx, dy, dz] = v[i[2] + dz, i[1] + dy, i[0] + dx]
        fx, fy, fz = f
        phi = _lerp(_lerp(_lerp(c[0, 0, 0], c[1, 0, 0], fx), _lerp(c[0, 1, 0], c[1, 1, 0], fx), fy),
                    _lerp(_lerp(c[0, 0, 1], c[1, 0, 1], fx), _lerp(c[0, 1, 1], c[1, 1, 1], fx), fy), fz)
        d = lambda p, q: (c[p] - c[q]).astype(F)
        Gx = _lerp(_lerp(d((1, 0, 0), (0, 0, 0)), d((1, 1, 0), (0, 1, 0)), fy), _lerp(d((1, 0, 1), (0, 0, 1)), d((1, 1, 1), (0, 1, 1)), fy), fz)
        Gy = _lerp(_lerp(d((0, 1, 0), (0, 0, 0)), d((1, 1, 0), (1, 0, 0)), fx), _lerp(d((0, 1, 1), (0, 0, 1)), d((1, 1, 1), (1, 0, 1)), fx), fz)
        Gz = _lerp(_lerp(d((0, 0, 1), (0, 0, 0)), d((1, 0, 1), (1, 0, 0)), fx), _lerp(d((0, 1, 1), (0, 1, 0)), d((1, 1, 1), (1, 1, 0)), fx), fy)
        grad = np.stack([(Gx * vol["inv"][0]).astype(F), (Gy * vol["inv"][1]).astype(F), (Gz * vol["inv"][2]).astype(F)], axis=1)
    return phi, grad, within


def sample_host_result(vol, l):
    """What sph_volume_sample_host returns: outside the extent phi is the quiet NaN 0x7FC00000 and the gradient zero."""
    phi, grad, within = sample(vol, l)
    phi = np.where(within, phi, np.array([0x7FC00000], np.uint32).view(F)[0]).astype(F)
    grad = np.where(within[:, None], grad, F(0)).astype(F)
    with np.errstate(invalid="ignore"):
        inside = within & (phi < 0)
    return phi, grad, inside


def _unit(g):
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot3(g[:, 0], g[:, 1], g[:, 2], g[:, 0], g[:, 1], g[:, 2])).astype(F)
        bad = (ln == 0) | ~np.isfinite(ln)
        m = (g / np.where(bad, F(1), ln)[:, None]).astype(F)
    return m, bad


def project(vol, l):
    """how (0 no hit, 1 projected, 2 the box decides), o (n, 3), m (n, 3) for local points l."""
    l = np.asarray(l, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        phi0, g0, within = sample(vol, l)
        hit = within & (phi0 < 0)
        m0, bad0 = _unit(g0)
        o1 = (l - (phi0[:, None] * m0).astype(F)).astype(F)
        phi1, g1, _ = sample(vol, o1, clamp=True)
        m1, bad1 = _unit(g1)
        o2 = (o1 - (phi1[:, None] * m1).astype(F)).astype(F)
        finite = np.isfinite(o2).all(axis=1)
    how = np.where(~hit, 0, np.where(bad0 | bad1, 2, np.where(finite, 1, 0)))
    return how, o2, m1


def hit(b, vol, mass, p, v, active):
    """obstacle_ref.hit for a box bound to `vol`: (p', v', inside, took the u_n < 0 branch, terms (n, 6) fp64)."""
    assert b["shape"] == R.BOX
    c, M, sz = b["c"], b["M"], b["size"]
    n = len(p)
    with np.errstate(all="ignore"):
        d = [(p[:, a] - c[a]).astype(F) for a in range(3)]
        l = [_dot3(d[0], d[1], d[2], np.full(n, M[j], F), np.full(n, M[3 + j], F), np.full(n, M[6 + j], F)) for j in range(3)]
        h = [F(sz[a]) for a in range(3)]
        al = [np.abs(l[a]) for a in range(3)]
        inbox = active & (al[0] < h[0]) & (al[1] < h[1]) & (al[2] < h[2])
        how, o2, m1 = project(vol, np.stack(l, axis=1))
        inside = inbox & (how != 0)
        gap = [(h[a] - al[a]).astype(F) for a in range(3)]
        cx = (gap[0] <= gap[1]) & (gap[0] <= gap[2])
        cy = ~cx & (gap[1] <= gap[2])
        pick = [cx, cy, ~cx & ~cy]
        o, m = [], []
        for a in range(3):
            s = np.where(l[a] >= 0, F(1), F(-1)).astype(F)
            ob = np.where(pick[a], (s * h[a]).astype(F), l[a]).astype(F)
            mb = np.where(pick[a], s, F(0)).astype(F)
            o.append(np.where(how == 1, o2[:, a], ob).astype(F))
            m.append(np.where(how == 1, m1[:, a], mb).astype(F))
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
    with np.errstate(all="ignore"):
        for a in range(3):
            J[:, a] = np.where(neg, m64 * (v[:, a].astype(np.float64) - v2[:, a].astype(np.float64)), 0.0)
        R64 = [np.asarray(x, np.float64) for x in rr]
        J[:, 3] = np.where(neg, R64[1] * J[:, 2] - R64[2] * J[:, 1], 0.0)
        J[:, 4] = np.where(neg, R64[2] * J[:, 0] - R64[0] * J[:, 2], 0.0)
        J[:, 5] = np.where(neg, R64[0] * J[:, 1] - R64[1] * J[:, 0], 0.0)
    return p2, v2, inside, neg, J


def apply(bs, vols, bindings, mass, rec):
    """obstacle_ref.apply with body k bound to vols[bindings[k]] (or to nothing: bindings[k] < 0)."""
    rec = rec.copy()
    p = rec["pos"][:, :3].astype(F).copy()
    v = rec["vel"][:, :3].astype(F).copy()
    active = (rec["isGhost"] == 0) & np.isfinite(p).all(axis=1)
    imp = np.zeros((len(bs), 6), np.float64)
    info = dict(touched=np.zeros(len(bs), np.int64), negative=np.zeros(len(bs), np.int64), abs_sum=np.zeros((len(bs), 6)), terms=[])
    for k, b in enumerate(bs):
        if bindings[k] >= 0:
            p, v, inside, neg, J = hit(b, vols[bindings[k]], mass, p, v, active)
        else:
            p, v, inside, neg, J = R.hit(b, mass, p, v, active)
        info["touched"][k] = int(inside.sum())
        info["negative"][k] = int(neg.sum())
        info["abs_sum"][k] = np.abs(J).sum(axis=0)
        info["terms"].append(J[inside])
        for a in range(6):
            imp[k, a] = math.fsum(J[inside, a])
    rec["pos"][:, :3] = p
    rec["vel"][:, :3] = v
    return rec, imp, info


def step(oracle, rec, op, bs, vols, bindings, dt=None):
    """One engine substep with bound bodies: (records, bodies, impulses, info)."""
    step_dt = F(op.timeStep if dt is None or dt <= 0 else dt)
    rec = oracle.substep(rec, op, dt=float(step_dt) if dt is not None and dt > 0 else -1.0)
    rec, imp, info = apply(bs, vols, bindings, F(op.mass), rec)
    return rec, R.advance(bs, step_dt), imp, info


# ---- mesh -> signed distance ------------------------------------------------------------------------
def lattice_points(origin, spacing, dims):
    """(n, 3) fp32 points origin + (float)i * spacing, x fastest, dims = (nx, ny, nz)."""
    o = np.asarray(origin, F)
    sp = np.broadcast_to(np.asarray(spacing, F), (3,)).astype(F)
    ax = [(o[a] + (np.arange(dims[a]).astype(F) * sp[a]).astype(F)).astype(F) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F)


def _d3(a, b):
    return _dot3(a[0], a[1], a[2], b[0], b[1], b[2])


def tri_d2(A, B, C, P):
    """Squared distance from points P (three fp32 arrays) to the triangle (A, B, C) (three fp32 scalars each): the region walk of 3f."""
    n = len(P[0])
    full = lambda s: np.full(n, s, F)
    ab = [full(F(B[i] - A[i])) for i in range(3)]
    ac = [full(F(C[i] - A[i])) for i in range(3)]
    bc = [full(F(C[i] - B[i])) for i in range(3)]
    with np.errstate(all="ignore"):
        ap = [(P[i] - A[i]).astype(F) for i in range(3)]
        bp = [(P[i] - B[i]).astype(F) for i in range(3)]
        cp = [(P[i] - C[i]).astype(F) for i in range(3)]
        d1, d2, d3, d4, d5, d6 = _d3(ab, ap), _d3(ac, ap), _d3(ab, bp), _d3(ac, bp), _d3(ab, cp), _d3(ac, cp)
        vc = ((d1 * d4).astype(F) - (d3 * d2).astype(F)).astype(F)
        vb = ((d5 * d2).astype(F) - (d1 * d6).astype(F)).astype(F)
        va = ((d3 * d6).astype(F) - (d5 * d4).astype(F)).astype(F)
        e43, e56 = (d4 - d3).astype(F), (d5 - d6).astype(F)
        r = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        t_ab = (d1 / (d1 - d3).astype(F)).astype(F)
        t_ac = (d2 / (d2 - d6).astype(F)).astype(F)
        t_bc = (e43 / (e43 + e56).astype(F)).astype(F)
        s = ((va + vb).astype(F) + vc).astype(F)
        fv, fw = (vb / s).astype(F), (vc / s).astype(F)
        q = []
        for i in range(3):
            cand = [full(A[i]), full(B[i]), (A[i] + (t_ab * ab[i]).astype(F)).astype(F), full(C[i]), (A[i] + (t_ac * ac[i]).astype(F)).astype(F),
                    (B[i] + (t_bc * bc[i]).astype(F)).astype(F)]
            out = ((A[i] + (ab[i] * fv).astype(F)).astype(F) + (ac[i] * fw).astype(F)).astype(F)
            for k in range(5, -1, -1):
                out = np.where(r[k], cand[k], out)
            q.append(out.astype(F))
        e = [(P[i] - q[i]).astype(F) for i in range(3)]
        return _d3(e, e)


def tri_angle64(A, B, C, P64):
    """atan2 term of the winding number in fp64 at points P64 (n, 3)."""
    a, b, c = np.asarray(A, np.float64) - P64, np.asarray(B, np.float64) - P64, np.asarray(C, np.float64) - P64
    la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
    det = np.einsum("ij,ij->i", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
    return np.arctan2(det, den)


def mesh_distance(vertices, triangles, origin, spacing, dims):
    """(signed distances (nz, ny, nx) fp32, winding number (n,) fp64): sqrtf(min d^2), negative where w >= 0.5."""
    V = np.asarray(vertices, F).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    pts = lattice_points(origin, spacing, dims)
    P = [pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()]
    P64 = pts.astype(np.float64)
    best = np.full(len(pts), np.inf, F)
    w = np.zeros(len(pts), np.float64)
    for t in T:
        A, B, C = V[t[0]], V[t[1]], V[t[2]]
        d2 = tri_d2(A, B, C, P)
        with np.errstate(invalid="ignore"):
            best = np.where(d2 < best, d2, best).astype(F)
        w += tri_angle64(A, B, C, P64)
    w /= 2.0 * np.pi
    d = np.sqrt(best).astype(F)
    out = np.where(w >= 0.5, -d, d).astype(F)
    return out.reshape(dims[2], dims[1], dims[0]), w


def brute_distance64(vertices, triangles, pts):
    """Unsigned distance in fp64 from pts (n, 3) to the mesh, by the same region walk."""
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    best = np.full(len(pts), np.inf)
    P = np.asarray(pts, np.float64)
    dot = lambda x, y: np.einsum("ij,ij->i", np.broadcast_to(x, P.shape), np.broadcast_to(y, P.shape))
    for t in np.asarray(triangles, np.int64).reshape(-1, 3):
        A, B, C = V[t[0]], V[t[1]], V[t[2]]
        ab, ac, bc = B - A, C - A, C - B
        ap, bp, cp = P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(all="ignore"):
            r = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            s = va + vb + vc
            q = A + ab * (vb / s)[:, None] + ac * (vc / s)[:, None]
            cand = [np.broadcast_to(A, P.shape), np.broadcast_to(B, P.shape), A + ab * (d1 / (d1 - d3))[:, None], np.broadcast_to(C, P.shape),
                    A + ac * (d2 / (d2 - d6))[:, None], B + bc * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None]]
            for k in range(5, -1, -1):
                q = np.where(r[k][:, None], cand[k], q)
            dd = np.linalg.norm(P - q, axis=1)
            best = np.where(dd < best, dd, best)
    return best


# ---- meshes built in code -------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(vertices (n, 3) fp32, triangles (m, 3) uint32), counter-clockwise seen from outside: 20 * 4^subdivisions triangles."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.array(v) * radius + np.asarray(center, np.float64)).astype(F)
    return verts, np.array(f, np.uint32)


def cube(half=1.0, center=(0.0, 0.0, 0.0)):
    """A cube of 12 triangles, counter-clockwise seen from outside."""
    s = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    tris = []
    for a, b, c, d in q:
        tris += [(a, b, c), (a, c, d)]
    return (s * half + np.asarray(center, np.float64)).astype(F), np.array(tris, np.uint32)


# ---- analytic lattices ------------------------------------------------------------------------------
def lattice_coords(n, spacing):
    """Local coordinates (fp64) of the n points of one axis of a centred lattice."""
    return (np.arange(n) - 0.5 * (n - 1)) * float(spacing)


def sphere_lattice(radius, spacing, margin=3):
    """Signed distances of a sphere about the lattice centre, (n, n, n) fp32, n odd."""
    n = 2 * (int(math.ceil(radius / spacing)) + margin) + 1
    a = lattice_coords(n, spacing)
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(F)


def box_lattice(half, spacing, margin=3, floor=None):
    """Signed distances of an axis-aligned box about the lattice centre, (nz, ny, nx) fp32; floor clamps the inside from below
    (a core of constant value: zero gradient)."""
    n = [2 * (int(math.ceil(half[a] / spacing)) + margin) + 1 for a in range(3)]
    z, y, x = np.meshgrid(lattice_coords(n[2], spacing), lattice_coords(n[1], spacing), lattice_coords(n[0], spacing), indexing="ij")
    q = [np.abs(x) - half[0], np.abs(y) - half[1], np.abs(z) - half[2]]
    outside = np.sqrt(sum(np.maximum(c, 0.0) ** 2 for c in q))
    inside = np.minimum(np.maximum(np.maximum(q[0], q[1]), q[2]), 0.0)
    phi = outside + inside
    if floor is not None:
        phi = np.maximum(phi, floor)
    return phi.astype(F)
