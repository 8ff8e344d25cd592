#!/usr/bin/env python3
"""Summary of tools/walk_l1_counters.sh: per engine build, the means over bench.py's timed launches of k_sph_walk of the L1 (TCP) counters
and the pass time.  usage: walk_l1_counters.py <dir with wl1_<lib>/ and wl1_<lib>.time> <out.json> <first launch> <launches> lib..."""
import glob
import importlib
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL = "k_sph_walk"
WAVES = 65536          # config 3: 4 194 304 targets, 64 per wave


def window(db, counter, first, count):
    """Per launch of the kernel (dispatch order): the counter summed over its instances; mean over launches [first, first + count)."""
    con = sqlite3.connect(db)
    per = {}
    for name, did, val in con.execute("select kernel_name, dispatch_id, value from counters_collection where counter_name = ?", (counter,)):
        if KERNEL in name:
            per[did] = per.get(did, 0.0) + val
    v = [per[d] for d in sorted(per)][first:first + count]
    return (sum(v) / len(v), len(v)) if v else (None, 0)


def main():
    d, out, first, count = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    pkg = importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd")
    rows = []
    for lib in sys.argv[5:]:
        row = {"build": lib}
        flags = os.path.join(ROOT, "variants", lib + ".flags")
        row["flags"] = open(flags).read().strip() if os.path.exists(flags) else ""
        try:
            row["sph_pass_us"] = json.loads(open(os.path.join(d, f"wl1_{lib}.time")).read().strip().splitlines()[-1])["us"].get("sph")
        except Exception as ex:                                  # noqa: BLE001
            row["sph_pass_us"] = None
            row["time_error"] = str(ex)
        dbs = glob.glob(os.path.join(d, f"wl1_{lib}", "**", "*.db"), recursive=True)
        for c, key in (("TCP_TCC_READ_REQ_sum", "l1_to_l2_read_requests"), ("TCP_TOTAL_CACHE_ACCESSES_sum", "l1_line_accesses"), ("TCP_CACHE_MISS", "l1_misses")):
            mean, n = window(dbs[0], c, first, count) if dbs else (None, 0)
            row[key + "_per_launch"] = mean
            row[key + "_per_wave"] = round(mean / WAVES, 1) if mean is not None else None
            row["launches"] = n
        a, m = row["l1_line_accesses_per_launch"], row["l1_misses_per_launch"]
        row["l1_hit_rate"] = round(1.0 - m / a, 4) if a and m is not None else None
        rows.append(row)
    res = {"workload": "config3", "kernel": KERNEL, "first_launch": first, "launches": count, "csrc_hash": pkg.build.csrc_hash(),
           "source": "tools/walk_l1_counters.sh: rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_CACHE_MISS (one pass per build) -- "
                     "python3 bench.py --steps 50 --warmup 5 --no-cpu-baseline --no-breakdown; the profiler offers no L1 hit counter on gfx950: "
                     "l1_hit_rate = 1 - TCP_CACHE_MISS / TCP_TOTAL_CACHE_ACCESSES; sph_pass_us from an untraced tools/time_kernels.py 3 3 50 5",
           "builds": rows}
    json.dump(res, open(out, "w"), indent=1)
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
