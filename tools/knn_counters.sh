#!/bin/bash
# Counter sets (one rocprofv3 --pmc pass each, nothing else traced) over k_knn and the neighbour list kernels on config 3 after 300
# substeps; means per launch.
# usage: knn_counters.sh <out dir> <tag> <k> <R over h> "<set 1>" "<set 2>" ...   -> <out dir>/<tag>_pmc.json
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$1; TAG=$2; K=$3; FAC=$4; shift 4
mkdir -p $OUT
i=0
for set in "$@"; do
  i=$((i+1)); rm -rf $OUT/${TAG}_$i
  timeout -k 10 240 rocprofv3 --pmc $set -d $OUT/${TAG}_$i -o p -- python3 $R/tools/knn_counters.py $K $FAC 5 > $OUT/${TAG}_$i.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "set $i ($set) failed with $rc"; exit $rc; fi
done
python3 - $OUT $TAG $K $FAC <<'PY'
import sqlite3, glob, sys, json
out = {"k": int(sys.argv[3]), "R_over_h": float(sys.argv[4]), "state": "config 3 after 300 substeps", "launches": "5 per kernel, means", "kernels": {}}
for db in sorted(glob.glob(f"{sys.argv[1]}/{sys.argv[2]}_*/**/*.db", recursive=True)):
    con = sqlite3.connect(db)
    tabs = [r[0] for r in con.execute("select name from sqlite_master where type='table' or type='view'")]
    t = [x for x in tabs if x.startswith("counters_collection")][0]
    acc = {}
    for n, c, v in con.execute(f"select kernel_name, counter_name, value from {t}"):
        for kern in ("k_knn", "k_neighbors_count", "k_neighbors_fill"):
            if kern + "<" in n or kern + "I" in n:
                acc.setdefault((kern, c), []).append(v)
    for (kern, c), vs in acc.items():
        out["kernels"].setdefault(kern, {})[c] = round(sum(vs) / len(vs), 1)
print(json.dumps(out))
open(f"{sys.argv[1]}/{sys.argv[2]}_pmc.json", "w").write(json.dumps(out, indent=1))
PY
