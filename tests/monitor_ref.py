"""A numpy restatement of the field monitors (include/sph_abi.h "field monitors"): the row update and the derived
fields in float64, in the stated order, every operation rounded on its own, and the rule for which substeps act and which ring row
they write.  Imported by the CPU and the GPU tests; no device and no library is needed."""
import numpy as np

ROW_DTYPE = np.dtype([("samples", "<u8"), ("wet", "<u8"), ("sumFraction", "<f8"), ("sumFraction2", "<f8"), ("sumDensity", "<f8"),
                      ("sumPressure", "<f8"), ("sumPressure2", "<f8"), ("sumVel", "<f8", (3,)), ("sumVelVel", "<f8", (6,))])
assert ROW_DTYPE.itemsize == 128
SAMPLE_DTYPE = np.dtype([("density", "<f4"), ("fraction", "<f4"), ("pressure", "<f4"), ("count", "<u4"), ("vel", "<f4", (3,)), ("pad", "<f4")])
assert SAMPLE_DTYPE.itemsize == 32
NO_ROW = 0xFFFFFFFF
(WET_SHARE, MEAN_FRACTION, VAR_FRACTION, MEAN_DENSITY, MEAN_PRESSURE, VAR_PRESSURE, MEAN_VEL_X, MEAN_VEL_Y, MEAN_VEL_Z, TKE) = range(10)
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))                  # sumVelVel: xx, yy, zz, xy, xz, yz


def update(rows, samples, wet_fraction=0.5):
    """One acting substep: `samples` (SAMPLE_DTYPE) into a copy of `rows` (ROW_DTYPE, None: zeros)."""
    s = np.ascontiguousarray(samples).view(SAMPLE_DTYPE).reshape(-1)
    r = np.zeros(len(s), ROW_DTYPE) if rows is None else np.ascontiguousarray(rows).view(ROW_DTYPE).reshape(-1).copy()
    f64 = np.float64
    fields = [s["density"], s["fraction"], s["pressure"], s["vel"][:, 0], s["vel"][:, 1], s["vel"][:, 2]]
    ok = np.ones(len(s), bool)
    for v in fields:
        ok &= np.isfinite(v)                                            # a sample with a non-finite field is skipped whole
    wet = ok & (s["fraction"] >= np.float32(wet_fraction))
    with np.errstate(all="ignore"):
        fr, de, pr = s["fraction"].astype(f64), s["density"].astype(f64), s["pressure"].astype(f64)
        v = s["vel"].astype(f64)
        r["samples"][ok] += 1
        r["sumFraction"][ok] = (r["sumFraction"] + fr)[ok]
        r["sumFraction2"][ok] = (r["sumFraction2"] + fr * fr)[ok]
        r["sumDensity"][ok] = (r["sumDensity"] + de)[ok]
        r["wet"][wet] += 1
        r["sumPressure"][wet] = (r["sumPressure"] + pr)[wet]
        r["sumPressure2"][wet] = (r["sumPressure2"] + pr * pr)[wet]
        for a in range(3):
            r["sumVel"][wet, a] = (r["sumVel"][:, a] + v[:, a])[wet]
        for k, (a, b) in enumerate(PAIRS):
            r["sumVelVel"][wet, k] = (r["sumVelVel"][:, k] + v[:, a] * v[:, b])[wet]
    return r


def _mean(total, n):
    with np.errstate(all="ignore"):
        return np.where(n > 0, total / np.where(n > 0, n, 1).astype(np.float64), 0.0)


def _var(total2, total, n):
    with np.errstate(all="ignore"):
        d = np.where(n > 0, n, 1).astype(np.float64)
        mean, second = total / d, total2 / d
        sq = mean * mean
        return np.where(n > 0, second - sq, 0.0)


def field(rows, which):
    """A derived field of ROW_DTYPE rows: float64 throughout, one rounding to float32 at the end."""
    r = np.ascontiguousarray(rows).view(ROW_DTYPE).reshape(np.shape(rows))
    n, w = r["samples"], r["wet"]
    if which == WET_SHARE:
        v = _mean(w.astype(np.float64), n)
    elif which == MEAN_FRACTION:
        v = _mean(r["sumFraction"], n)
    elif which == VAR_FRACTION:
        v = _var(r["sumFraction2"], r["sumFraction"], n)
    elif which == MEAN_DENSITY:
        v = _mean(r["sumDensity"], n)
    elif which == MEAN_PRESSURE:
        v = _mean(r["sumPressure"], w)
    elif which == VAR_PRESSURE:
        v = _var(r["sumPressure2"], r["sumPressure"], w)
    elif which in (MEAN_VEL_X, MEAN_VEL_Y, MEAN_VEL_Z):
        v = _mean(r["sumVel"][..., which - MEAN_VEL_X], w)
    elif which == TKE:
        xx, yy, zz = (_var(r["sumVelVel"][..., a], r["sumVel"][..., a], w) for a in range(3))
        v = 0.5 * ((xx + yy) + zz)
    else:
        raise ValueError(which)
    with np.errstate(all="ignore"):
        return v.astype(np.float32)


def acts(c, every):
    """Does substep number c (0-based, counted since the set or reset) act?"""
    return c % every == 0


def ring_row(a, history, stride):
    """The ring row acting substep number a (0-based) writes, or NO_ROW."""
    return (a // stride) % history if history > 0 and a % stride == 0 else NO_ROW


def schedule(every, stride, history, substeps):
    """(acts, rows) of the first `substeps` substeps, as sph_monitor_schedule_host gives them."""
    out_a, out_r, a = [], [], 0
    for c in range(substeps):
        if acts(c, every):
            out_a.append(1)
            out_r.append(ring_row(a, history, stride))
            a += 1
        else:
            out_a.append(0)
            out_r.append(NO_ROW)
    return np.array(out_a, np.uint32), np.array(out_r, np.uint32)


def ring_span(acting, history, stride):
    """(index of the oldest ring row held, rows held) after `acting` acting substeps."""
    taken = (acting + stride - 1) // stride if history else 0
    have = min(taken, history)
    return taken - have, have


def random_samples(rng, m, wet_fraction=0.5, hard=True):
    """m samples like the sampler's, with (hard) the cases the contract names: exact ties at wet_fraction, -0.0, NaN / inf fields
    (skipped whole), all-zero records and large-magnitude values with full mantissas (their products must be exact)."""
    s = np.zeros(m, SAMPLE_DTYPE)
    s["density"] = rng.uniform(0.0, 2000.0, m)
    s["fraction"] = rng.uniform(0.0, 1.2, m)
    s["pressure"] = rng.normal(0.0, 3.0e4, m)
    s["count"] = rng.integers(0, 60, m)
    s["vel"] = rng.normal(0.0, 30.0, (m, 3))
    if hard:
        k = rng.integers(0, 12, m)
        s["fraction"][k == 0] = np.float32(wet_fraction)                # an exact tie is wet
        s["fraction"][k == 1] = np.nextafter(np.float32(wet_fraction), np.float32(-1))
        s["vel"][k == 2] = np.float32(-0.0)
        s["pressure"][k == 2] = np.float32(-0.0)
        s["pressure"][k == 3] = np.nan
        s["vel"][k == 4, 1] = np.inf
        s["density"][k == 5] = -np.inf
        s[k == 6] = np.zeros(1, SAMPLE_DTYPE)[0]                         # a dry, all-zero record
        big = k == 7                                                     # full 24-bit mantissas at 2^40 and at 2^-40
        s["vel"][big] = (rng.integers(2 ** 23, 2 ** 24, (int(big.sum()), 3)) * rng.choice([-1.0, 1.0], (int(big.sum()), 3))).astype(np.float32) * np.float32(2.0 ** 17)
        s["pressure"][big] = rng.integers(2 ** 23, 2 ** 24, int(big.sum())).astype(np.float32) * np.float32(2.0 ** 20)
        small = k == 8
        s["vel"][small] = rng.integers(2 ** 23, 2 ** 24, (int(small.sum()), 3)).astype(np.float32) * np.float32(2.0 ** -63)
        s["fraction"][k == 9] = np.nan
    return s
