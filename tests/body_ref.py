"""Numpy restatement of the dynamic rigid bodies (include/sph_abi.h "dynamic rigid bodies") and of the moments of a
lattice body.

It builds on obstacle_ref: a body is obstacle_ref's dict of fp32 arrays, the pose advance is obstacle_ref.advance.  fp32 with the correctly
rounded fma of obstacle_ref wherever the engine has one (dot3 only), every other fp32 operation rounded on its own (numpy float32 scalars);
fp64 where the engine uses fp64 (the J and L terms, the inversion of the inertia on set); math.fsum for the moments.

record(d): a DYNAMICS_DTYPE record -> dict (None for mass 0: kinematic).  world(...): what the step needs of the scene.
step(b, d, S, W, dt): one body, one substep (steps 1 to 7 of section 3g).  step_all(): a set.  moments(): the ten moments of a lattice.
"""
from __future__ import annotations

import math

import numpy as np

import obstacle_ref as R

F = np.float32
D = np.float64
DYNAMICS_DTYPE = np.dtype([("mass", "<f4"), ("inertia", "<f4", (6,)), ("com", "<f4", (3,)), ("gravityScale", "<f4"), ("force", "<f4", (3,)),
                           ("torque", "<f4", (3,)), ("linearDamping", "<f4"), ("angularDamping", "<f4"), ("flags", "<u4")])
CONFINED = 1


def _fma(a, b, c):
    return F(np.asarray(R._fma(F(a), F(b), F(c))).reshape(-1)[0])


def dot3(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, F(ax) * F(bx)))


def invert_inertia(inertia):
    """The fp64 inverse (adjugate over determinant, the engine's expressions) of the fp32 tensor, rounded to fp32; None if not positive definite."""
    xx, yy, zz, xy, xz, yz = (float(F(x)) for x in inertia)
    m2 = xx * yy - xy * xy
    c00, c01, c02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    det = xx * c00 + xy * c01 + xz * c02
    if not (xx > 0.0 and m2 > 0.0 and det > 0.0 and math.isfinite(det)):
        return None
    return np.array([c00 / det, (xx * zz - xz * xz) / det, m2 / det, c01 / det, c02 / det, (xy * xz - xx * yz) / det], D).astype(F)


def record(d):
    d = np.asarray(d, DYNAMICS_DTYPE).reshape(())
    if float(d["mass"]) == 0.0:
        return None
    return dict(mass=F(d["mass"]), I=d["inertia"].astype(F).copy(), Iinv=invert_inertia(d["inertia"]), com=d["com"].astype(F).copy(),
                gscale=F(d["gravityScale"]), force=d["force"].astype(F).copy(), torque=d["torque"].astype(F).copy(),
                ldamp=F(d["linearDamping"]), adamp=F(d["angularDamping"]), flags=int(d["flags"]))


def world(gravity, box_center, axes9, half, restitution):
    """axes9: the container's rotation as the engine holds it (pkg.rotation_mat3: axis j in world coordinates is axes9[3 j : 3 j + 3])."""
    return dict(g=np.asarray(gravity, F), bc=np.asarray(box_center, F), A=np.asarray(axes9, F).reshape(9), half=np.asarray(half, F), rest=F(restitution))


def sym_world(M, S, x):
    """M (S (M^T x)), S = (xx, yy, zz, xy, xz, yz): three rows of dot3 each."""
    l0 = dot3(x[0], x[1], x[2], M[0], M[3], M[6])
    l1 = dot3(x[0], x[1], x[2], M[1], M[4], M[7])
    l2 = dot3(x[0], x[1], x[2], M[2], M[5], M[8])
    s0 = dot3(S[0], S[3], S[4], l0, l1, l2)
    s1 = dot3(S[3], S[1], S[5], l0, l1, l2)
    s2 = dot3(S[4], S[5], S[2], l0, l1, l2)
    return [dot3(M[0], M[1], M[2], s0, s1, s2), dot3(M[3], M[4], M[5], s0, s1, s2), dot3(M[6], M[7], M[8], s0, s1, s2)]


def cross(a, b):
    a = [F(x) for x in a]
    b = [F(x) for x in b]
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def support(b):
    """(local support points in their fixed order, radius)."""
    sz = [F(x) for x in b["size"]]
    z = F(0)
    if b["shape"] == R.SPHERE:
        return [[z, z, z]], sz[0]
    if b["shape"] == R.CAPSULE:
        return [[z, -sz[1], z], [z, sz[1], z]], sz[0]
    return [[sz[0] if i & 1 else -sz[0], sz[1] if i & 2 else -sz[1], sz[2] if i & 4 else -sz[2]] for i in range(8)], z


def step(b, d, S, W, dt, info=None):
    """One substep of one dynamic body with the substep's sums S = (J, L) about the geometric centre: the new body.  info (a dict) receives
    the faces in contact and the intermediates of the linear update."""
    dt = F(dt)
    M = [F(x) for x in b["M"]]
    S = [float(x) for x in S]
    com = [F(x) for x in d["com"]]
    with np.errstate(all="ignore"):
        # 1. to the centre of mass
        o = [dot3(M[0], M[1], M[2], *com), dot3(M[3], M[4], M[5], *com), dot3(M[6], M[7], M[8], *com)]
        O = [float(x) for x in o]
        Lg = [F(S[3] - (O[1] * S[2] - O[2] * S[1])), F(S[4] - (O[2] * S[0] - O[0] * S[2])), F(S[5] - (O[0] * S[1] - O[1] * S[0]))]
        w = [F(x) for x in b["w"]]
        x = cross(w, o)
        Vg = [F(b["v"][a]) + x[a] for a in range(3)]
        # 2. linear velocity
        mass = F(d["mass"])
        inter = []
        for a in range(3):
            acc = d["gscale"] * F(W["g"][a]) + F(d["force"][a]) / mass
            jm = F(S[a] / float(mass))
            t1 = Vg[a] + jm
            push = dt * acc
            inter.append((float(Vg[a]), float(jm), float(t1), float(push)))
            Vg[a] = t1 + push
        # 3. angular velocity
        Iw = sym_world(M, d["I"], w)
        gy = cross(w, Iw)
        rhs = [Lg[a] + dt * (F(d["torque"][a]) - gy[a]) for a in range(3)]
        dw = sym_world(M, d["Iinv"], rhs)
        w = [w[a] + dw[a] for a in range(3)]
        # 4. damping
        fl = max(F(0), F(1) - d["ldamp"] * dt)
        fa = max(F(0), F(1) - d["adamp"] * dt)
        Vg = [v * fl for v in Vg]
        w = [v * fa for v in w]
        # 5. container contact at the entry pose
        c = [F(v) for v in b["c"]]
        faces = []
        if d["flags"] & CONFINED:
            lp, rad = support(b)
            pen = [F(0)] * 6
            im = F(1) / mass
            ope = F(1) + W["rest"]
            A = [F(v) for v in W["A"]]
            for f in range(6):
                j = f >> 1
                sg = F(-1) if f & 1 else F(1)
                n = [sg * A[3 * j], sg * A[3 * j + 1], sg * A[3 * j + 2]]
                for p in lp:
                    s = [dot3(M[0], M[1], M[2], *p), dot3(M[3], M[4], M[5], *p), dot3(M[6], M[7], M[8], *p)]
                    r = [s[a] - o[a] for a in range(3)]
                    dd = [(c[a] + s[a]) - F(W["bc"][a]) for a in range(3)]
                    dist = F(W["half"][j]) + dot3(dd[0], dd[1], dd[2], n[0], n[1], n[2])
                    depth = rad - dist
                    if not depth >= 0:
                        continue
                    if depth > pen[f]:
                        pen[f] = depth
                    wr = cross(w, r)
                    vn = dot3(Vg[0] + wr[0], Vg[1] + wr[1], Vg[2] + wr[2], n[0], n[1], n[2])
                    if not vn < 0:
                        continue
                    rn = cross(r, n)
                    k3 = sym_world(M, d["Iinv"], rn)
                    kr = cross(k3, r)
                    den = im + dot3(n[0], n[1], n[2], kr[0], kr[1], kr[2])
                    jn = (-ope * vn) / den
                    jm = jn * im
                    Vg = [Vg[a] + jm * n[a] for a in range(3)]
                    w = [w[a] + jn * k3[a] for a in range(3)]
            for f in range(6):
                if not pen[f] > 0:
                    continue
                faces.append(f)
                j = f >> 1
                sg = F(-1) if f & 1 else F(1)
                c = [c[a] + pen[f] * (sg * A[3 * j + a]) for a in range(3)]
        # 6. back to the geometric centre
        x = cross(w, o)
        V = [Vg[a] - x[a] for a in range(3)]
    if info is not None:
        info["faces"] = faces
        info["linear"] = inter
    nb = dict(b, c=np.array(c, F), v=np.array(V, F), w=np.array(w, F))
    # 7. the pose advance of section 3e with the new velocities
    return R.advance([nb], dt)[0]


def step_all(bs, ds, imp, W, dt, infos=None):
    """One substep of a set: dynamic bodies step, kinematic ones (record None) advance.  imp: (K, 6) sums of this substep or None."""
    out = []
    for i, (b, d) in enumerate(zip(bs, ds)):
        if d is None:
            out.append(R.advance([b], F(dt))[0])
        else:
            info = {} if infos is not None else None
            out.append(step(b, d, np.zeros(6) if imp is None else imp[i], W, dt, info))
            if infos is not None:
                infos.append(info)
    return out


def moment_terms(values, spacing):
    """Per lattice point the ten fp64 terms of the moments ((n, 10), points in memory order), the cell volume, and the cell diagonal D.
    values: (nz, ny, nx) fp32."""
    v = np.ascontiguousarray(values, F)
    nz, ny, nx = v.shape
    sp = np.broadcast_to(np.asarray(spacing, F), (3,)).astype(F)
    half = [F(F(0.5) * F(n - 1)) * sp[a] for a, n in enumerate((nx, ny, nz))]
    diag = F(np.sqrt(dot3(sp[0], sp[1], sp[2], sp[0], sp[1], sp[2])))
    lx = ((np.arange(nx, dtype=F) * sp[0]).astype(F) - half[0]).astype(F)
    ly = ((np.arange(ny, dtype=F) * sp[1]).astype(F) - half[1]).astype(F)
    lz = ((np.arange(nz, dtype=F) * sp[2]).astype(F) - half[2]).astype(F)
    with np.errstate(all="ignore"):
        q = (F(0.5) - (v / diag).astype(F)).astype(F)
    w32 = np.where(np.isnan(q), F(0), np.minimum(np.maximum(q, F(0)), F(1))).astype(F)
    w = w32.astype(D)
    X = np.broadcast_to(lx.astype(D)[None, None, :], v.shape)
    Y = np.broadcast_to(ly.astype(D)[None, :, None], v.shape)
    Z = np.broadcast_to(lz.astype(D)[:, None, None], v.shape)
    wx, wy, wz = w * X, w * Y, w * Z
    t = np.stack([w, wx, wy, wz, wx * X, wy * Y, wz * Z, wx * Y, wx * Z, wy * Z], axis=-1).reshape(-1, 10)
    cell = (float(sp[0]) * float(sp[1])) * float(sp[2])
    return t, cell, float(diag)


def moments(values, spacing):
    """(the ten moments with correctly rounded sums, the order bound 2 (n - 1) 2^-53 sum |t| cell per moment)."""
    t, cell, _ = moment_terms(values, spacing)
    sums = np.array([math.fsum(t[:, c]) for c in range(10)])
    bound = 2.0 * (len(t) - 1) * 2.0 ** -53 * np.abs(t).sum(axis=0) * cell
    return sums * cell, bound
