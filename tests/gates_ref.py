"""Numpy restatement of the flow gates (include/sph_abi.h "flow gates"): what crosses an oriented planar patch
between the entry and the exit state of one substep, written from the contract (not from the kernel).

fp32 with scalar_ref.fma32 / dot3 wherever section 3r has an fma (the two sides, the intersection point, the patch coordinates, the
ellipse test), every other operation rounded on its own.  A gate is a record of GATE_DTYPE.
step(): the books of one substep from 80-byte entry and exit records in index order, the sums taken by math.fsum, with sum |term| per
sum for coupling_ref.books_bound.
"""
from __future__ import annotations

import math

import numpy as np

from coupling_ref import books_bound
from scalar_ref import dot3, fma32

F = np.float32
RECT, ELLIPSE = 0, 1
UNBOUNDED = 1
GATE_DTYPE = np.dtype([("shape", "<i4"), ("flags", "<i4"), ("center", "<f4", (3,)), ("u", "<f4", (3,)), ("v", "<f4", (3,)), ("pad", "<f4", (5,))])
assert GATE_DTYPE.itemsize == 64
CHANNELS = 4


def gate(shape, center, u, v, unbounded=False):
    g = np.zeros(1, GATE_DTYPE)[0]
    g["shape"], g["flags"] = shape, UNBOUNDED if unbounded else 0
    g["center"], g["u"], g["v"] = center, u, v
    return g


def gate_box(center, half):
    """Six rectangles with outward normals (-x, +x, -y, +y, -z, +z)."""
    out = []
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        for sign in (-1.0, 1.0):
            ce, u, v = np.array(center, np.float64), np.zeros(3), np.zeros(3)
            ce[a] += sign * half[a]
            u[b], v[d] = half[b], sign * half[d]
            out.append(gate(RECT, ce, u, v))
    return out


def normal(g):
    """cross(u, v): per component a multiply, a multiply and a subtract."""
    u, v = g["u"].astype(F), g["v"].astype(F)
    return np.array([F(F(u[1] * v[2]) - F(u[2] * v[1])), F(F(u[2] * v[0]) - F(u[0] * v[2])), F(F(u[0] * v[1]) - F(u[1] * v[0]))], F)


def _full(n, x):
    return np.full(n, F(x), F)


def side(g, pos):
    """dot3(p - center, N) per particle ((n, 3) fp32 positions)."""
    n, N, c = len(pos), normal(g), g["center"].astype(F)
    with np.errstate(all="ignore"):
        d = [(pos[:, a].astype(F) - c[a]).astype(F) for a in range(3)]
        return dot3(d[0], d[1], d[2], _full(n, N[0]), _full(n, N[1]), _full(n, N[2]))


def targets(entry, exit_):
    """Records the step looks at: isGhost == 0 and a finite position at the entry and at the exit."""
    return (exit_["isGhost"] == 0) & np.isfinite(exit_["pos"][:, :3]).all(axis=1) & np.isfinite(entry["pos"][:, :3]).all(axis=1)


def in_patch(g, p0, p1, s0, s1):
    """Does the segment meet the plane inside the patch (strict), per particle."""
    n = len(p0)
    if int(g["flags"]) & UNBOUNDED:
        return np.ones(n, bool)
    c, u, v = g["center"].astype(F), g["u"].astype(F), g["v"].astype(F)
    one = np.ones(1, F)
    uu = dot3(u[0] * one, u[1] * one, u[2] * one, u[0] * one, u[1] * one, u[2] * one)[0]
    vv = dot3(v[0] * one, v[1] * one, v[2] * one, v[0] * one, v[1] * one, v[2] * one)[0]
    with np.errstate(all="ignore"):
        t = (s0 / (s0 - s1).astype(F)).astype(F)
        d = [(fma32(t, (p1[:, a] - p0[:, a]).astype(F), p0[:, a]) - c[a]).astype(F) for a in range(3)]
        a = dot3(d[0], d[1], d[2], _full(n, u[0]), _full(n, u[1]), _full(n, u[2]))
        b = dot3(d[0], d[1], d[2], _full(n, v[0]), _full(n, v[1]), _full(n, v[2]))
        if int(g["shape"]) == ELLIPSE:
            fa, fb = (a / uu).astype(F), (b / vv).astype(F)
            return fma32(fa, fa, (fb * fb).astype(F)) < F(1.0)
        return (np.abs(a) < uu) & (np.abs(b) < vv)


def crossings(g, entry, exit_):
    """(forward mask, backward mask) of the counted crossers of one gate."""
    p0, p1 = entry["pos"][:, :3].astype(F), exit_["pos"][:, :3].astype(F)
    s0, s1 = side(g, p0), side(g, p1)
    with np.errstate(all="ignore"):
        fw, bw = (s0 < 0) & (s1 >= 0), (s0 >= 0) & (s1 < 0)
        ok = targets(entry, exit_) & (fw | bw)
        ok &= in_patch(g, p0, p1, s0, s1)
    return fw & ok, bw & ok


def step(entry, exit_, gates, values=None):
    """The books of one substep: forward / backward (G,) counts, vel (G, 3) and scalar (G, 4) sums (math.fsum, correctly rounded) and
    abs_vel / abs_scalar, the sums of |term|, for the bound between two fp64 sums of the same terms in different orders."""
    G = len(gates)
    c = None if values is None else np.ascontiguousarray(values, F).reshape(len(exit_), -1)
    out = dict(forward=np.zeros(G, np.uint64), backward=np.zeros(G, np.uint64), vel=np.zeros((G, 3)), scalar=np.zeros((G, CHANNELS)),
               abs_vel=np.zeros((G, 3)), abs_scalar=np.zeros((G, CHANNELS)))
    for i, g in enumerate(gates):
        fw, bw = crossings(g, entry, exit_)
        sign = np.where(fw, 1.0, -1.0)[fw | bw]
        out["forward"][i], out["backward"][i] = int(fw.sum()), int(bw.sum())
        v = exit_["vel"][:, :3].astype(np.float64)[fw | bw]
        for a in range(3):
            out["vel"][i, a] = math.fsum(sign * v[:, a])
            out["abs_vel"][i, a] = math.fsum(np.abs(v[:, a]))
        if c is not None:
            cc = c[fw | bw].astype(np.float64)
            cc = np.where(np.isfinite(cc), cc, 0.0)
            for k in range(c.shape[1]):
                out["scalar"][i, k] = math.fsum(sign * cc[:, k])
                out["abs_scalar"][i, k] = math.fsum(np.abs(cc[:, k]))
    return out


def add(total, books):
    """Accumulate one substep's books (step()) into a running total (None: start one)."""
    if total is None:
        return {k: v.copy() for k, v in books.items()}
    for k in total:
        total[k] = total[k] + books[k]
    return total


def above(g, rec):
    """Records on the forward side (s >= 0) of a gate's plane among those with isGhost == 0 and a finite position."""
    ok = (rec["isGhost"] == 0) & np.isfinite(rec["pos"][:, :3]).all(axis=1)
    with np.errstate(all="ignore"):
        return ok & (side(g, rec["pos"][:, :3].astype(F)) >= 0)


# ---- what the CPU and the GPU tests share ------------------------------------------------------------
def check_books(got, want, what):
    """Counts exactly, sums within the bound of two fp64 sums of the same terms in different orders."""
    assert got["forward"].tolist() == want["forward"].tolist() and got["backward"].tolist() == want["backward"].tolist(), what
    hits = want["forward"] + want["backward"]
    for name in ("vel", "scalar"):
        bound = books_bound(hits[:, None], want["abs_" + name])
        err = np.abs(got[name] - want[name])
        assert (err <= bound).all(), f"{what}: {name} error {err.max():.3g} above {bound.max():.3g}"


def mixed_gates(pkg, center, size):
    """Eight gates of mixed shapes around `center`: tilted rectangles and ellipses, two whole planes, one far outside (empty)."""
    c = np.asarray(center, np.float64)
    s = float(size)
    rot = lambda a, b, t: (np.cos(t) * a + np.sin(t) * b, -np.sin(t) * a + np.cos(t) * b)
    ex, ey, ez = np.eye(3)
    u1, v1 = rot(ex, ey, 0.3)
    u2, v2 = rot(ey, ez, -0.7)
    return [pkg.gate(pkg.SPH_GATE_RECT, c, 0.5 * s * ex, 0.4 * s * ez),
            pkg.gate(pkg.SPH_GATE_ELLIPSE, c + 0.1 * s * ey, 0.45 * s * ez, 0.3 * s * ex),
            pkg.gate(pkg.SPH_GATE_RECT, c, 0.3 * s * u1, 0.6 * s * ez),
            pkg.gate(pkg.SPH_GATE_ELLIPSE, c - 0.2 * s * ex, 0.5 * s * u2, 0.25 * s * v2),
            pkg.gate(pkg.SPH_GATE_RECT, c, ex, ez, unbounded=True),
            pkg.gate(pkg.SPH_GATE_ELLIPSE, c + 0.05 * s * ex, 2.0 * v1, 3.0 * ez, unbounded=True),
            pkg.gate(pkg.SPH_GATE_RECT, c + 100.0 * s * ey, 0.5 * s * ex, 0.5 * s * ez),
            pkg.gate(pkg.SPH_GATE_RECT, c - 0.3 * s * ey, 0.05 * s * ez, 0.6 * s * ex)]
