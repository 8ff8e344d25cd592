"""The geometric statement of a ray cast in float64, all pairs: the sphere entered first inside [tmin, tmax], ordered by (t, id).  It
also NAMES the rays it cannot vouch for against an fp32 implementation: the two smallest t within 1e-5 relative of each other, any
sphere grazed (|s| < 1e-5 r^2), an entry within 1e-5 relative of tmin or tmax."""
import numpy as np

EPS = 1e-5


def void(r):
    r = np.asarray(r, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (r[:, 4:7].astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)
        bad = ~np.isfinite(r[:, 0:7]).all(axis=1) | np.isnan(r[:, 7]) | ~(a > 0) | ~np.isfinite(a) | (r[:, 3] > r[:, 7])
    return bad


def cast(pos, r, radius, takes_part=None, chunk=256):
    """(t (m,) float64 (+inf: a miss), ids (m,) int64 (-1), named (m,) bool) of rays r (m, 8) against spheres of `radius` at pos (n, 3)."""
    x = np.asarray(pos, np.float64)[:, :3]
    n = len(x)
    part = np.ones(n, bool) if takes_part is None else np.asarray(takes_part, bool)
    r = np.asarray(r, np.float32)
    m = len(r)
    t_out, id_out, named = np.full(m, np.inf), np.full(m, -1, np.int64), np.zeros(m, bool)
    bad = void(r)
    r2 = float(radius) ** 2
    for lo in range(0, m, chunk):
        rr = r[lo:lo + chunk].astype(np.float64)
        ok_ray = ~bad[lo:lo + chunk]
        o, d, tmin, tmax = rr[:, 0:3], rr[:, 4:7], rr[:, 3], rr[:, 7]
        with np.errstate(all="ignore"):
            a = (d * d).sum(axis=1)
            L = x[None, :, :] - o[:, None, :]
            tca = (L * d[:, None, :]).sum(axis=2) / a[:, None]
            q = L - tca[:, :, None] * d[:, None, :]
            s = r2 - (q * q).sum(axis=2)
            t = tca - np.sqrt(np.maximum(s, 0.0) / a[:, None])
            ok = (s >= 0) & (t >= tmin[:, None]) & (t <= tmax[:, None]) & part[None, :] & ok_ray[:, None]
            tt = np.where(ok, t, np.inf)
            order = np.argsort(tt, axis=1, kind="stable")[:, :2]                 # stable: equal t keep ascending id
            rows = np.arange(len(rr))
            t1 = tt[rows, order[:, 0]]
            t2 = tt[rows, order[:, 1]] if n > 1 else np.full(len(rr), np.inf)
            hit = np.isfinite(t1)
            t_out[lo:lo + chunk] = t1
            id_out[lo:lo + chunk] = np.where(hit, order[:, 0], -1)
            close = hit & np.isfinite(t2) & (t2 - t1 <= EPS * np.maximum(np.abs(t1), np.abs(t2)))
            graze = ((np.abs(s) < EPS * r2) & part[None, :]).any(axis=1)
            edge_lo = np.abs(t - tmin[:, None]) <= EPS * np.maximum(np.abs(t), np.abs(tmin[:, None]))
            edge_hi = np.isfinite(tmax[:, None]) & (np.abs(t - tmax[:, None]) <= EPS * np.maximum(np.abs(t), np.abs(tmax[:, None])))
            edge = ((s >= 0) & part[None, :] & (edge_lo | edge_hi)).any(axis=1)
            named[lo:lo + chunk] = ok_ray & (close | graze | edge)
    return t_out, id_out, named
