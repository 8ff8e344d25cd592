"""numpy restatement of the state statistics, written from DESIGN.md section 3c (not from the kernels).

Inputs: the 80-byte records, the members (SphParams), the grid (SphGridInfo) and each particle's cell (download_grid()'s
particle_cell, which the parity tests pin to the oracle's BuildGrid; this also settles where a NaN position is binned).
`statistics` returns a dict of plain numpy values; `pack` lays it out as the ctypes struct so tests can compare bytes."""
import numpy as np

F = np.float32
TILE = 2048
NONE = 0xFFFFFFFF
SUM_NAMES = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "speed2", "density", "density2", "pressure", "foam", "inv_density",
             "ang_x", "ang_y", "ang_z")
# roundings inside one term (conversions fp32 -> fp64 and products of two fp32 factors are exact)
TERM_ROUNDINGS = {"pos_x": 0, "pos_y": 0, "pos_z": 0, "vel_x": 0, "vel_y": 0, "vel_z": 0, "speed2": 2, "density": 0, "density2": 0,
                  "pressure": 0, "foam": 0, "inv_density": 1, "ang_x": 5, "ang_y": 5, "ang_z": 5}
DENSITY, PRESSURE, SPEED, POS_X, POS_Y, POS_Z, FOAM = range(7)


def sets(rec):
    """(fluid, active ghost, inactive ghost, other, non-finite fluid, counted) masks."""
    g, a = rec["isGhost"], rec["isActive"]
    fluid = g == 0
    ag = (g == 1) & (a != 0)
    ig = (g == 1) & (a == 0)
    other = ~(fluid | ag | ig)
    fin = (np.isfinite(rec["pos"][:, :3]).all(axis=1) & np.isfinite(rec["vel"][:, :3]).all(axis=1) & np.isfinite(rec["density"]) &
           np.isfinite(rec["pressure"]) & np.isfinite(rec["padA"]))
    return fluid, ag, ig, other, fluid & ~fin, fluid & fin


def speed2_f32(rec):
    v = rec["vel"].astype(F)
    with np.errstate(all="ignore"):
        return ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)


def terms(rec, counted, center):
    """The 15 fp64 terms per record (record order), +0.0 outside the counted set."""
    with np.errstate(all="ignore"):
        x, y, z = (rec["pos"][:, a].astype(np.float64) for a in range(3))
        vx, vy, vz = (rec["vel"][:, a].astype(np.float64) for a in range(3))
        r = rec["density"].astype(np.float64)
        dx, dy, dz = x - float(F(center[0])), y - float(F(center[1])), z - float(F(center[2]))
        t = {
            "pos_x": x, "pos_y": y, "pos_z": z, "vel_x": vx, "vel_y": vy, "vel_z": vz,
            "speed2": (vx * vx + vy * vy) + vz * vz,
            "density": r, "density2": r * r, "pressure": rec["pressure"].astype(np.float64), "foam": rec["padA"].astype(np.float64),
            "inv_density": np.where(rec["density"] > 0, 1.0 / r, 0.0),
            "ang_x": dy * vz - dz * vy, "ang_y": dz * vx - dx * vz, "ang_z": dx * vy - dy * vx,
        }
    return {k: np.where(counted, v, 0.0) for k, v in t.items()}


def tree_depth(n):
    """Additions on the path of one term: 11 inside the tile plus log2 of the padded tile count."""
    nt = -(-n // TILE)
    t2 = 1
    while t2 < nt:
        t2 *= 2
    return 11 + (t2.bit_length() - 1)


def tree_sum(x):
    """Sum of a 1-D float64 sequence in the contract's order: tiles of 2048 padded with +0.0, halving x[i] += x[i + s] for
    s = 1024 .. 1 inside a tile, then the tile sums padded with +0.0 to a power of two and the same halving."""
    n = len(x)
    nt = -(-n // TILE)
    if nt == 0:
        return np.float64(0.0)
    t = np.zeros(nt * TILE, np.float64)
    t[:n] = x
    t = t.reshape(nt, TILE)
    h = TILE // 2
    while h >= 1:
        t = t[:, :h] + t[:, h:2 * h]
        h //= 2
    t2 = 1
    while t2 < nt:
        t2 *= 2
    y = np.zeros(t2, np.float64)
    y[:nt] = t[:, 0]
    while len(y) > 1:
        h = len(y) // 2
        y = y[:h] + y[h:]
    return y[0]


def _extreme(values, ids, is_min):
    """(value with its stored bits, id): fp32 compare, lowest id among records that compare equal."""
    if len(values) == 0:
        return F(np.inf) if is_min else F(-np.inf), NONE
    m = values.min() if is_min else values.max()
    i = ids[values == m].min()
    return values[ids == i][0], int(i)


def histogram(values, bins, lo, hi):
    """bins + 2 uint64 slots of fp32 `values`: v < lo -> 0, v >= hi -> bins + 1, else 1 + min(floor((v - lo) * (bins / (hi - lo))), bins - 1)."""
    v = np.asarray(values, F)
    lo, hi = F(lo), F(hi)
    scale = F(bins) / (hi - lo)
    with np.errstate(all="ignore"):
        f = np.floor(((v - lo) * scale).astype(F))
    mid = 1 + np.minimum(np.where(np.isfinite(f), f, 0).astype(np.int64), bins - 1)
    slot = np.where(v < lo, 0, np.where(v >= hi, bins + 1, mid))
    return np.bincount(slot, minlength=bins + 2).astype(np.uint64)


def field_values(rec, field):
    if field == SPEED:
        return np.sqrt(speed2_f32(rec)).astype(F)
    return {DENSITY: rec["density"], PRESSURE: rec["pressure"], POS_X: rec["pos"][:, 0], POS_Y: rec["pos"][:, 1], POS_Z: rec["pos"][:, 2],
            FOAM: rec["padA"]}[field].astype(F)


def statistics(rec, params, grid, particle_cell, specs=()):
    n = len(rec)
    ids = np.arange(n, dtype=np.int64)
    fluid, ag, ig, other, bad, counted = sets(rec)
    out = {"numRecords": n, "numFluid": int(fluid.sum()), "numActiveGhosts": int(ag.sum()), "numInactiveGhosts": int(ig.sum()),
           "numOther": int(other.sum()), "numNonFinite": int(bad.sum()), "numCounted": int(counted.sum())}
    gmin = np.array(list(grid.gridMin), F)
    dims = np.array(list(grid.dims))
    with np.errstate(all="ignore"):
        q = np.floor(((rec["pos"][:, :3].astype(F) - gmin) / F(grid.cellSize)).astype(F))
        esc = counted & ((q < 0) | (q >= dims.astype(F))).any(axis=1)
    out["numEscaped"] = int(esc.sum())
    out["firstNonFiniteId"] = int(ids[bad].min()) if bad.any() else NONE
    out["firstEscapedId"] = int(ids[esc].min()) if esc.any() else NONE
    cid = ids[counted]
    c = rec[counted]
    s2 = speed2_f32(rec)[counted]
    for a in range(3):
        out[f"minPos{a}"] = _extreme(c["pos"][:, a], cid, True)
        out[f"maxPos{a}"] = _extreme(c["pos"][:, a], cid, False)
    out["minDensity"] = _extreme(c["density"], cid, True)
    out["maxDensity"] = _extreme(c["density"], cid, False)
    out["minPressure"] = _extreme(c["pressure"], cid, True)
    out["maxPressure"] = _extreme(c["pressure"], cid, False)
    out["maxFoam"] = _extreme(c["padA"], cid, False)
    out["maxSpeed2"] = _extreme(s2, cid, False)
    out["maxSpeed"] = F(np.sqrt(out["maxSpeed2"][0])) if len(cid) else F(0)
    order = np.lexsort((ids, np.asarray(particle_cell, np.int64)))          # cell ascending, id ascending inside a cell
    t = terms(rec, counted, params.param_boxCenter)
    out["sums"] = {k: tree_sum(t[k][order]) for k in SUM_NAMES}
    occ = np.bincount(np.asarray(particle_cell, np.int64), minlength=grid.numCells) if n else np.zeros(grid.numCells, np.int64)
    out["occupiedCells"] = int((occ > 0).sum())
    out["maxCellCount"] = int(occ.max())
    out["maxCellIndex"] = int(np.argmax(occ))                              # argmax: the first, i.e. lowest, index
    out["occupancy"] = np.bincount(np.minimum(occ, 64), minlength=65).astype(np.uint64)
    out["histograms"] = [histogram(field_values(rec, f)[counted], b, lo, hi) for f, b, lo, hi in specs]
    return out


def pack(ref, struct_type):
    """The restatement's result laid out as the ctypes mirror of SphStatistics."""
    s = struct_type()
    for k in ("numRecords", "numFluid", "numActiveGhosts", "numInactiveGhosts", "numOther", "numNonFinite", "numCounted", "numEscaped",
              "firstNonFiniteId", "firstEscapedId", "occupiedCells", "maxCellCount", "maxCellIndex"):
        setattr(s, k, ref[k])

    def put(dst, pair):
        dst.value = float(pair[0])                      # (a float32 survives the round trip through a Python float, -0.0 included)
        dst.id = pair[1]
    for a in range(3):
        put(s.minPos[a], ref[f"minPos{a}"])
        put(s.maxPos[a], ref[f"maxPos{a}"])
    for k in ("minDensity", "maxDensity", "minPressure", "maxPressure", "maxFoam", "maxSpeed2"):
        put(getattr(s, k), ref[k])
    s.maxSpeed = float(ref["maxSpeed"])
    sm = ref["sums"]
    for a, ax in enumerate("xyz"):
        s.sumPos[a] = sm["pos_" + ax]
        s.sumVel[a] = sm["vel_" + ax]
        s.sumAngular[a] = sm["ang_" + ax]
    s.sumSpeed2, s.sumDensity, s.sumDensity2 = sm["speed2"], sm["density"], sm["density2"]
    s.sumPressure, s.sumFoam, s.sumInvDensity = sm["pressure"], sm["foam"], sm["inv_density"]
    for m in range(65):
        s.occupancy[m] = int(ref["occupancy"][m])
    return s


def to_bytes(ref, struct_type):
    return bytes(pack(ref, struct_type)) + b"".join(h.tobytes() for h in ref["histograms"])


def host_cells(rec, grid):
    """BuildGrid's clamped cell of every record, for CPU tests that have no engine to ask (finite positions only)."""
    gmin = np.array(list(grid.gridMin), F)
    dims = np.array(list(grid.dims))
    q = np.floor(((rec["pos"][:, :3].astype(F) - gmin) / F(grid.cellSize)).astype(F))
    q = np.minimum(np.maximum(q, F(0)), (dims - 1).astype(F)).astype(np.int64)
    return (q[:, 2] * dims[1] + q[:, 1]) * dims[0] + q[:, 0]
