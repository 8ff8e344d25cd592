"""Timing of the state statistics (include/sph_abi.h "statistics") at BASELINE.json configs[2] (4 M particles,
128^3 cells), on the lattice state (after 1 substep) and after 300 substeps (the compressed regime):

  (a) the grid build the call starts with: device time of the classes bin + scan + scatter under SPH_OPT_TIMING
  (b) the statistics kernels alone (class "other": k_stats_tiles, k_stats_cells, k_stats_finish, and k_stats_hist with histograms),
      without histograms and with four 256-bin histograms
  (c) the whole sph_statistics call, wall time, without and with the histograms
  (d) what a caller had before, in the same run: f.download() alone, wall, and f.download() plus the numpy reductions that give the
      same numbers (counts, extrema with ids, the fp64 sums, cell occupancy)

5 warm-up calls, median and p10-p90 of 25.
  python tools/time_statistics.py [out.json]
Without an argument the result goes to time_statistics.json in the current directory; profiles/r07_time_statistics.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys
import time

import numpy as np

import timing
from timing import pkg, stats


def numpy_reductions(rec, g):
    """The numbers of SphStatistics from downloaded records with plain numpy (np.sum's own order, not the contract's)."""
    fl = rec["isGhost"] == 0
    p, v = rec["pos"][:, :3], rec["vel"][:, :3]
    fin = np.isfinite(p).all(axis=1) & np.isfinite(v).all(axis=1) & np.isfinite(rec["density"]) & np.isfinite(rec["pressure"]) & np.isfinite(rec["padA"])
    c = rec[fl & fin]
    p, v = c["pos"][:, :3], c["vel"][:, :3]
    out = [len(c), p.min(axis=0), p.argmin(axis=0), p.max(axis=0), p.argmax(axis=0), c["density"].min(), c["density"].argmin(), c["density"].max(),
           c["density"].argmax(), c["pressure"].min(), c["pressure"].max(), c["padA"].max()]
    s2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    out += [s2.max(), s2.argmax()]
    p64, v64, r64 = p.astype(np.float64), v.astype(np.float64), c["density"].astype(np.float64)
    out += [p64.sum(axis=0), v64.sum(axis=0), (v64 * v64).sum(), r64.sum(), (r64 * r64).sum(), c["pressure"].astype(np.float64).sum(),
            c["padA"].astype(np.float64).sum(), (1.0 / r64).sum(), np.cross(p64, v64).sum(axis=0)]
    q = np.floor((p - np.array(list(g.gridMin), np.float32)) / np.float32(g.cellSize))
    dims = np.array(list(g.dims))
    out.append(int(((q < 0) | (q >= dims)).any(axis=1).sum()))
    q = np.clip(q, 0, dims - 1).astype(np.int64)
    occ = np.bincount((q[:, 2] * dims[1] + q[:, 1]) * dims[0] + q[:, 0], minlength=g.numCells)
    out += [np.bincount(np.minimum(occ, 64), minlength=65), occ.max(), occ.argmax()]
    return out


def main() -> None:
    out_path = timing.out_path(sys.argv[1:], "statistics")
    cfg, rec, sp = timing.config3()
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    g = f.ComputeGridExtents()
    head = timing.header("tools/time_statistics.py", cfg, rec, grid=list(g.dims))
    del rec
    rho0, half = float(sp.param_restDensity), float(sp.param_boxHalf[1])
    specs = [(pkg.SPH_STAT_DENSITY, 256, 0.0, 16 * rho0), (pkg.SPH_STAT_PRESSURE, 256, 0.0, 4.0e7), (pkg.SPH_STAT_SPEED, 256, 0.0, 120.0),
             (pkg.SPH_STAT_POS_Y, 256, -half, half)]
    reps, warm = 25, 5

    def wall(fn, reps=reps, warm=warm):
        for _ in range(warm):
            fn()
        us = []
        for _ in range(reps):
            f.sync()
            t0 = time.perf_counter()
            fn()
            us.append((time.perf_counter() - t0) * 1e6)
        return stats(us)

    def classes(hist):
        """Device time per call of the grid build classes and of class "other" (SPH_OPT_TIMING)."""
        f.set_option(pkg.SPH_OPT_TIMING, 1)
        for _ in range(warm):
            f.statistics(hist)
        f.kernel_times(reset=True)
        build, other, launches = [], [], []
        for _ in range(reps):
            f.statistics(hist)
            kt = f.kernel_times(reset=True)
            build.append((kt["bin"][0] + kt["scan"][0] + kt["scatter"][0]) * 1000.0)
            other.append(kt["other"][0] * 1000.0)
            launches.append(int(kt["other"][1]))
        f.set_option(pkg.SPH_OPT_TIMING, 0)
        return stats(build), dict(stats(other), launches_per_call=int(np.median(launches)))

    res = dict(head, histograms=[list(s) for s in specs], regimes={})
    for label, substep, _ in timing.regimes(f):                          # (downloads: lazy AoS mode writes the records back once, outside the timings)
        r = {}
        r["a_grid_build"], r["b_statistics_kernels"] = classes(None)
        _, r["b_statistics_kernels_4x256_bins"] = classes(specs)
        r["c_statistics_call_wall"] = wall(lambda: f.statistics())
        r["c_statistics_call_wall_4x256_bins"] = wall(lambda: f.statistics(specs))
        r["d_download_wall"] = wall(lambda: f.download(), reps=7, warm=2)
        r["d_download_plus_numpy_wall"] = wall(lambda: numpy_reductions(f.download(), g), reps=5, warm=1)
        s = f.statistics(specs)
        r["kernels_over_grid_build"] = r["b_statistics_kernels"]["median_us"] / r["a_grid_build"]["median_us"]
        r["kernels_4x256_bins_over_grid_build"] = r["b_statistics_kernels_4x256_bins"]["median_us"] / r["a_grid_build"]["median_us"]
        r["download_over_call"] = r["d_download_wall"]["median_us"] / r["c_statistics_call_wall"]["median_us"]
        r["download_plus_numpy_over_call"] = r["d_download_plus_numpy_wall"]["median_us"] / r["c_statistics_call_wall"]["median_us"]
        r["state"] = {"counted": int(s.numCounted), "max_speed": float(s.maxSpeed), "cfl": s.cfl, "mean_density_over_rho0": s.mean_density / rho0,
                      "max_density_over_rho0": float(s.maxDensity.value) / rho0, "occupied_cells": int(s.occupiedCells),
                      "max_cell_count": int(s.maxCellCount), "cells_with_64_or_more": int(s.occupancy[64]),
                      "histogram_inside_fraction": [float(h[1:-1].sum()) / max(int(h.sum()), 1) for h in s.histograms]}
        res["regimes"][label] = dict(substep=substep, **r)
        print(label, json.dumps({k: (x["median_us"] if isinstance(x, dict) and "median_us" in x else x) for k, x in r.items()}), flush=True)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
