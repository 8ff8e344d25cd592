"""Numpy restatement of ray_span (include/sph_abi.h "ray spans") over all pairs, in fp32 operation by operation: every operation
rounded on its own, dot3 and the foot of the centre through fma32 (a correctly rounded fmaf), IEEE division and square root.  It gives
the bytes of sph_rays_span_host: tEnter, tExit, idEnter, idExit, count, flags and length per ray, from min, max and integer sums."""
import numpy as np

from diffuse_crest_ref import fma32
from rays_ref import void
import rays_scenes as RS

F = np.float32
INFO_FIELDS = ("rays", "crossed", "voidRays", "total", "maxCount", "radius", "flags")


def _ordered(f):
    """float32 -> uint32 in the order of the floats (negative below positive): the cast's key map."""
    u = np.ascontiguousarray(f, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def _dot3(ax, ay, az, bx, by, bz):
    return fma32(az, bz, fma32(ay, by, (ax * bx).astype(F)))


def spans(pos, r, radius, dtype, takes_part=None, chunk=128):
    """Rows of `dtype` (RAY_SPAN_DTYPE) of rays r (m, 8) against spheres of `radius` at pos (n, 3), takes_part (n,) bool."""
    x = np.asarray(pos, F)[:, :3]
    n = len(x)
    part = np.ones(n, bool) if takes_part is None else np.asarray(takes_part, bool)
    x, ids = x[part], np.flatnonzero(part).astype(np.uint64)
    r = np.asarray(r, F)
    m = len(r)
    out = np.zeros(m, dtype)
    out["tEnter"], out["tExit"], out["idEnter"], out["idExit"] = np.inf, -np.inf, -1, -1
    bad = void(r)
    out["flags"] = bad
    r2 = F(F(radius) * F(radius))
    if not len(x):
        return out
    with np.errstate(all="ignore"):
        for lo in range(0, m, chunk):
            rr = r[lo:lo + chunk]
            k = len(rr)
            o, d, tmin, tmax = rr[:, None, 0:3], rr[:, None, 4:7], rr[:, None, 3], rr[:, None, 7]
            dx, dy, dz = (np.broadcast_to(d[..., a], (k, len(x))) for a in range(3))
            a = _dot3(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2])
            inva = (F(1.0) / a).astype(F)
            L = (x[None, :, :] - o).astype(F)
            tca = (_dot3(L[..., 0], L[..., 1], L[..., 2], dx, dy, dz) * inva).astype(F)
            q = [fma32(-tca, (dx, dy, dz)[c], L[..., c]) for c in range(3)]
            s = (r2 - _dot3(q[0], q[1], q[2], q[0], q[1], q[2])).astype(F)
            thc = np.sqrt((s * inva).astype(F)).astype(F)
            tin = np.fmax((tca - thc).astype(F), tmin).astype(F)
            tout = np.fmin((tca + thc).astype(F), tmax).astype(F)
            ok = (s >= 0) & (tin < tout) & ~bad[lo:lo + chunk, None]
            f = np.fmin(((tout - tin).astype(F) / (F(2.0) * thc).astype(F)).astype(F), F(1.0)).astype(F)
            qq = np.where(ok, fma32(f, np.full_like(f, 16777216.0), np.full_like(f, 0.5)), F(0)).astype(np.uint64)   # (truncation of a value >= 0)
            count = ok.sum(axis=1)
            ke = np.where(ok, (_ordered(tin) << np.uint64(32)) | ids[None, :], np.uint64(0xFFFFFFFFFFFFFFFF))
            kx = np.where(ok, (_ordered(tout) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids[None, :]), np.uint64(0))
            je, jx = ke.argmin(axis=1), kx.argmax(axis=1)
            rows = np.arange(k)
            hit = count > 0
            blk = out[lo:lo + chunk]
            blk["tEnter"] = np.where(hit, tin[rows, je], F(np.inf))
            blk["tExit"] = np.where(hit, tout[rows, jx], F(-np.inf))
            blk["idEnter"] = np.where(hit, ids[je].astype(np.int64), -1)
            blk["idExit"] = np.where(hit, ids[jx].astype(np.int64), -1)
            blk["count"] = count
            blk["length"] = qq.sum(axis=1, dtype=np.uint64)
            out[lo:lo + chunk] = blk
    return out


def takes_part(rec, grid, fluid_only=False):
    """Participation: floorf((x - gridMin) / cellSize) in [0, dims) on every axis in fp32; without ghosts under fluid_only."""
    lo, dims, cs = grid
    with np.errstate(all="ignore"):
        c = np.floor(((rec["pos"][:, :3].astype(F) - np.asarray(lo, F)).astype(F) / F(cs)).astype(F))
        ok = ((c >= 0) & (c < np.asarray(dims, F))).all(axis=1)
    return ok & ~((rec["isGhost"] != 0) & bool(fluid_only))


# ---- what the span tests share ----------------------------------------------------------------------
def same_rows(got, want, what):
    """RAY_SPAN_DTYPE rows byte for byte; names the first rays that differ."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(len(got), 8) != want.view(np.uint32).reshape(len(want), 8)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[:5].tolist()}: {got[bad[:3]].tolist()} against {want[bad[:3]].tolist()}")


def info_of_rows(rows, info, what):
    """The info's sums are the sums over the rows."""
    assert info.rays == len(rows) and info.crossed == (rows["count"] > 0).sum() and info.voidRays == (rows["flags"] & 1).sum(), what
    assert info.total == rows["count"].astype(np.uint64).sum() and info.maxCount == (rows["count"].max() if len(rows) else 0), what


_SCENES = None


def scenes(pkg):
    """rays_scenes.scenes(pkg) without the entries that ask for any_hit (fluid_only kept), built once."""
    global _SCENES
    if _SCENES is None:
        _SCENES = [(name, rec, sp, [(r, radius, kw) for r, radius, kw in casts if not kw.get("any_hit")]) for name, rec, sp, casts in RS.scenes(pkg)]
    return _SCENES


def far_or_lat(pkg, r):
    """The `far` and `lat` families of rays_scenes.scenes: tmin = 0 and tmax = +inf on every ray, and starts outside the container box
    (the `inside` family has the same window and starts inside it)."""
    if not len(r) or not ((r[:, 3] == 0).all() and np.isposinf(r[:, 7]).all()):
        return False
    sp = RS.params(pkg)
    c, half = np.array(list(sp.param_boxCenter), F), np.array(list(sp.param_boxHalf), F)
    return bool((np.abs(r[:, 0:3] - c) > half).any(axis=1).mean() > 0.9)


def first_entry(pkg, rec, sp, r, radius, rows, hits, what, exact=False):
    """tEnter / idEnter of span rows against the (t, ids, ...) of a cast of the same rays, all of which have tmin = 0, tmax = +inf.
    The two are the same bytes except where the two definitions differ, and each differing ray must be one of these:
      graze   the cast's first sphere has no chord of positive length in fp32 (s == 0, or tca - thc == tca + thc): the cast hits it,
              a span does not cross it, so tEnter is a later sphere's, at or behind the cast's t
      inside  the ray starts inside a sphere: the cast ignores it, a span counts it with tEnter == tmin
    Measured on the host twins: lattice, lat, r = 0.125: 43 of 684 grazes (rays along lattice lines touch whole rows in one point each);
    r = 0.25: 10; dense lattice, lat: 71 grazes; dense lattice, far: 1 of 1024 starts inside (that lattice fills the grid).
    exact: no exception at all (the uniform cloud: generic positions, starts outside)."""
    t, ids = hits[0], hits[1]
    bad = np.flatnonzero((rows["tEnter"].view(np.uint32) != np.ascontiguousarray(t).view(np.uint32)) | (rows["idEnter"] != ids))
    print(what, "rays", len(r), "first entry differs from the cast on", len(bad))
    if exact:
        assert not len(bad), f"{what}: tEnter / idEnter differ from the cast on rays {bad[:5].tolist()}"
    for i in bad:
        inside = rows["tEnter"][i] == r[i, 3] and rows["count"][i] > 0
        graze = ids[i] >= 0 and pkg.ray_spans_host(rec[ids[i]:ids[i] + 1], sp, r[i:i + 1], radius)["count"][0] == 0 and rows["tEnter"][i] >= t[i]
        assert inside or graze, f"{what}: ray {i}: span {rows[i]} against the cast's t {t[i]} id {ids[i]}"
