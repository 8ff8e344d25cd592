"""Timing of the connected components (include/sph_abi.h "connected components") at config 3 (4 M particles, 128^3 cells,
h = cellSize), at substep 0 and after 300 substeps with a wave impulse on the way, at R = h and R = 2h.

A build synchronises once per round, so device events around a call would time the host as well.  The numbers are the engine's own
brackets (SPH_OPT_TIMING, class `other`: one bracket per launch of a build, so the bracket count is the number of launches), a series
of calls after warm-ups per variant:

  components       sph_components_build(R, SPH_COMPONENTS_FLUID_ONLY): time, rounds, launches, bodies
  full_walk        the same with SPH_OPT_COMPONENTS_VARIANT 1 (the hook walks every candidate, not only j < q)
  lane_atomics     the same with SPH_OPT_COMPONENTS_VARIANT 2 (the table kernel issues its atomics per lane); few calls: on one body of
                   millions every atomic lands on one row
  count_only       sph_neighbors_build(R, COUNT_ONLY) in the same run: ids + count walk + scan
  grid_build       bin + scan + scatter classes of the same calls (what every build runs first)

One hook round does one count walk's loads: per_round_over_count = (components / rounds) / count_only and whole_over_count =
components / count_only are the two ratios of DESIGN.md section 6.
  python tools/time_components.py [out.json]
Without an argument the result goes to time_components.json in the current directory.
"""
from __future__ import annotations

import functools
import json
import sys

import timing
from timing import components_build as components, pkg

REPS = 10
series = functools.partial(timing.series, reps=REPS, warm=2)


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "components")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    h = sp.param_h
    res = timing.header("tools/time_components.py", cfg, rec, reps=REPS, regimes={})
    done = 0
    for label, substep in (("substep_0", 0), ("after_300_with_wave", 300)):
        if substep > done:
            f.DispatchN(100)
            f.ApplyWaveImpulse(60.0, 3.0, 0.25, (0.0, 1.0, 0.0))
            f.DispatchN(substep - done - 100)
            done = substep
        f.sync()
        r = {}
        for name, R in (("R=h", h), ("R=2h", 2.0 * h)):
            v = {}
            cnt, grid_us = series(f, lambda: timing.neighbors_build(f, R, pkg.SPH_NEIGHBORS_COUNT_ONLY))
            launches = []
            full, _ = series(f, lambda: components(f, R), launches=launches)
            info = f.component_info()
            v["count_only"], v["grid_build"], v["components"] = cnt, grid_us, full
            v.update(rounds=int(info.rounds), launches=launches[-1], bodies=int(info.numComponents), largest=int(info.largestCount),
                     singletons=int(info.numSingletons), excluded=int(info.numExcluded))
            v["per_round_over_count"] = full["median_us"] / info.rounds / cnt["median_us"]
            v["whole_over_count"] = full["median_us"] / cnt["median_us"]
            f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, 1)
            v["full_walk"], _ = series(f, lambda: components(f, R), reps=5, warm=1)
            v["full_walk_rounds"] = int(f.component_info().rounds)
            f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, 2)
            v["lane_atomics"], _ = series(f, lambda: components(f, R), reps=2, warm=0)
            f.set_option(pkg.SPH_OPT_COMPONENTS_VARIANT, 0)
            r[name] = v
            print(label, name, json.dumps({k: (x["median_us"] if isinstance(x, dict) else x) for k, x in v.items()}), flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
