"""Timing of the neighbour lists (include/sph_abi.h "fixed-radius neighbour lists") at config 3 (4 M particles, 128^3 cells,
h = cellSize), on the lattice state and after 300 substeps (the compressed regime), at R = h and R = 2h, for the
default lists, SPH_NEIGHBORS_HALF and SPH_NEIGHBORS_COUNT_ONLY.

A build synchronises (the index buffer is sized from the total), so device events around a call would time the host as well.  The
numbers here are the engine's own brackets instead (SPH_OPT_TIMING, class `other`, which holds nothing but the neighbour kernels
during these calls: ids, count, the three scan kernels, fill), one series of 25 calls after 3 warm-ups per variant:

  count_only     ids + count + scan
  full           ids + count + scan + fill                 fill  = full - count_only   (medians)
  full_wave_fill the same with SPH_OPT_NEIGHBORS_FILL 1 (the wave-cooperative row write; same bits)
  scan_floor     a COUNT_ONLY query of n all-NaN points: ids + a count kernel that walks nothing + the scan of n rows
                                                           count = count_only - scan_floor
  yardstick      sph_sample_points_device at the particles' own positions (code of the parent commit): the same s = 1 candidate rows,
                 32 bytes written per target; count and fill are reported as ratios to it
  grid_build     bin + scan + scatter classes of the same calls (what every build runs first)

Entries per second = total / fill; the fill's store bandwidth = 4 bytes * total / fill.
  python tools/time_neighbors.py [out.json]
Without an argument the result goes to time_neighbors.json in the current directory; profiles/r15_time_neighbors.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import neighbors_build as build, neighbors_query_count as query_count, pkg, series


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "neighbors")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    n = len(rec)
    h = sp.param_h
    CO = pkg.SPH_NEIGHBORS_COUNT_ONLY
    nan_pts = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
    samples = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    res = timing.header("tools/time_neighbors.py", cfg, rec, reps=timing.REPS, regimes={})
    for label, substep, state in timing.regimes(f, (("lattice_state", 0), ("compressed", 300))):
        own = torch.from_numpy(np.ascontiguousarray(state["pos"])).cuda()
        torch.cuda.synchronize()
        r = {}
        yard, grid_us = series(f, lambda: f.sample_device(own.data_ptr(), n, samples.data_ptr()))
        r["yardstick_sample_points_at_particles"] = yard
        r["grid_build"] = grid_us
        for name, R in (("R=h", h), ("R=2h", 2.0 * h)):
            v = {}
            floor, _ = series(f, lambda: query_count(f, nan_pts, R))
            cnt, _ = series(f, lambda: build(f, R, CO))
            v["scan_floor"], v["count_only"] = floor, cnt
            v["count_us"] = cnt["median_us"] - floor["median_us"]
            v["count_over_yardstick"] = v["count_us"] / yard["median_us"]
            for variant, fl in (("default", 0), ("half", pkg.SPH_NEIGHBORS_HALF)):
                c, _ = series(f, lambda: build(f, R, fl | CO)) if fl else (cnt, None)
                full, _ = series(f, lambda: build(f, R, fl))
                f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 1)
                wave, _ = series(f, lambda: build(f, R, fl))
                f.set_option(pkg.SPH_OPT_NEIGHBORS_FILL, 0)
                info = f.neighbor_info()
                fill_us = full["median_us"] - c["median_us"]
                wave_us = wave["median_us"] - c["median_us"]
                v[variant] = dict(full=full, count_only=c, total=int(info.total), max_count=int(info.maxCount), mean_degree=info.total / n,
                                  full_wave_fill=wave, wave_fill_us=wave_us, wave_fill_store_GBps=4.0 * info.total / (wave_us * 1e-6) / 1e9,
                                  fill_us=fill_us, fill_over_yardstick=fill_us / yard["median_us"],
                                  entries_per_s=info.total / (fill_us * 1e-6), fill_store_GBps=4.0 * info.total / (fill_us * 1e-6) / 1e9)
            r[name] = v
        res["regimes"][label] = dict(substep=substep, **r)
        brief = {"yardstick_us": yard["median_us"], "grid_build_us": grid_us["median_us"]}
        for name in ("R=h", "R=2h"):
            v = r[name]
            brief[name] = {"count_us": v["count_us"], "scan_floor_us": v["scan_floor"]["median_us"],
                           **{k: {"fill_us": v[k]["fill_us"], "wave_fill_us": v[k]["wave_fill_us"], "total": v[k]["total"], "GBps": v[k]["fill_store_GBps"]} for k in ("default", "half")}}
        print(label, json.dumps(brief), flush=True)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
