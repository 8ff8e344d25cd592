"""Timing of the crest births of the diffuse pool (include/sph_abi.h "births at wave crests") at config 3 (4 M
particles, 128^3 cells, h = cellSize) after 300 substeps (the compressed regime), at R = h and R = 2h, all in
ONE process on ONE state.

The numbers are the engine's own brackets (SPH_OPT_TIMING, class `other`, one bracket per substep).  SPH_OPT_DIFFUSE_TIMED 2 puts the
pool's bracket around its spawn side, which the crest term's launches are part of (pass 1 by slot, the scan and compaction of the shell
slots, pass 2, then count, scans, compaction, emit, ticks); the advance kernel, which the term does not touch, is outside.

  pool[R].crest_off        the spawn side of a substep with the crest term off
  pool[R].every_1          ... with the term on and acting on every substep
  pool[R].every_4          ... with every = 4: `acting` the substeps whose counter is a multiple of 4, `idle` the others (the same
                           launches, the two passes return at once), `mean_us` over all of them
  query_build[R]           sph_shell_build at the same R in the same run, whole (ids, k_shell_gather, two scans and compactions,
                           k_shell_crest; one host synchronisation in the middle): the yardstick
  added_us                 every_1 - crest_off (medians): what an acting substep pays for the term
  added_over_query_build   added_us / query_build median: the in-substep pass does the same two walks with a third of pass 1's output
                           bytes and no scan of rows by id, so this should not exceed 1
  idle_added_us            every_4.idle - crest_off: what a substep that does not act pays for the fixed launch list

  python tools/time_crest.py [out.json]
Without an argument the result goes to time_crest.json in the current directory; profiles/r22_time_crest.json is the committed record.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import other_us, pkg, series, shell_build, stats

C_POOL = 1 << 20
REPS = 24                                                                        # a multiple of 4: six acting substeps at every = 4
PROBE = np.zeros((1, 3), np.float32)


def pool_series(e, state, reps=REPS, warm=4):
    """(microseconds of the pool's bracket, the pool's counter before the substep) of `reps` single dispatches after `warm` warm-ups.
    The fluid's state is uploaded again in front of every dispatch (an upload does not touch the pool): every substep walks the very
    state the query is built on, whose shell and degrees decide what both cost."""
    def rewind():
        e.upload(state)
        e.sample(PROBE)                                                          # (takes the uploaded records in: the dispatch's bracket stays the pool's alone)
        other_us(e)
    for _ in range(warm):
        rewind()
        e.DispatchCompute()
    us, counters = [], []
    for _ in range(reps):
        counters.append(e.diffuse_info()["substeps"])
        rewind()
        e.DispatchCompute()
        t, brackets = other_us(e)
        assert brackets == 1, brackets
        us.append(t)
    return us, counters


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "crest")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    h = sp.param_h
    res = timing.header("tools/time_crest.py", cfg, rec, capacity=C_POOL, reps=REPS, regimes={})
    for label, substep, state in timing.regimes(f, (("compressed", 300),)):
        r = {}
        e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
        e.set_option(pkg.SPH_OPT_TIMING, 1)
        e.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, 2)
        e.set_diffuse(capacity=C_POOL)
        for name, R in (("R=h", h), ("R=2h", 2.0 * h)):
            v = {}
            query, _ = series(f, lambda: shell_build(f, R))
            si = f.shell_info()
            v["query_build"] = dict(query, num_shell=int(si.numShell), shell_share=si.numShell / len(state), stencil=int(si.stencil))
            e.clear_diffuse_crest()
            off, _ = pool_series(e, state)
            v["crest_off"] = stats(off)
            e.set_diffuse_crest(radius=float(R), every=1)
            before = e.diffuse_crest_info()
            on, _ = pool_series(e, state)
            after = e.diffuse_crest_info()
            v["every_1"] = dict(stats(on), shell_size=after["shellSize"], shell_is_the_querys=after["shellSize"] == int(si.numShell), stencil=after["stencil"],
                                crest_born_per_substep=(after["crestSpawned"] - before["crestSpawned"]) / max(1, after["acting"] - before["acting"]))
            e.set_diffuse_crest(radius=float(R), every=4)
            us, counters = pool_series(e, state)
            acting = [t for t, c in zip(us, counters) if c % 4 == 0]
            idle = [t for t, c in zip(us, counters) if c % 4 != 0]
            v["every_4"] = dict(acting=stats(acting), idle=stats(idle), mean_us=sum(us) / len(us))
            v["added_us"] = v["every_1"]["median_us"] - v["crest_off"]["median_us"]
            v["added_over_query_build"] = v["added_us"] / query["median_us"]
            v["idle_added_us"] = v["every_4"]["idle"]["median_us"] - v["crest_off"]["median_us"]
            info = e.diffuse_info()
            v["pool_alive"] = info["alive"]
            print(label, name, json.dumps({k: (x["median_us"] if isinstance(x, dict) and "median_us" in x else x) for k, x in v.items() if k != "every_4"}),
                  "every 4:", v["every_4"]["acting"]["median_us"], v["every_4"]["idle"]["median_us"], flush=True)
            r[name] = v
        e.close()
        res["regimes"][label] = dict(substep=substep, **r)
    res["bench"] = "bench.py sets no pool: it runs the launches it ran before"
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
