#!/bin/bash
# L1 <-> L2 traffic of k_sph_walk over exactly bench.py's timed launches, for engine builds under variants/ ("default" = the in-tree library):
# L1->L2 read requests, L1 line accesses and L1 misses per launch (one rocprofv3 --pmc pass per build, the three TCP counters in one group),
# plus the pass time of the same launches from the engine's own events (an untraced run).
# usage (on a GPU box): bash tools/walk_l1_counters.sh <out.json> lib...     (build the variants first: tools/build_variant.sh)
#   intermediate files go to $WL1_DIR (default: build/wl1 under the repository, which git ignores)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "$1"); shift
D=$(realpath -m "${WL1_DIR:-$R/build/wl1}")
K=50; W=5
CMD="python3 $R/bench.py --steps $K --warmup $W --no-cpu-baseline --no-breakdown"
T=$(mktemp -d)
mkdir -p $D && cd $T && export TMPDIR=$T
for lib in "$@"; do
  if [ "$lib" = default ]; then unset SPH_HIP_LIB; else export SPH_HIP_LIB=$R/variants/$lib.so; fi
  echo "== $lib: time" | tee -a $D/wl1_progress.log
  timeout -k 10 200 python3 $R/tools/time_kernels.py 3 3 $K $W > $D/wl1_$lib.time 2> $D/wl1_$lib.time.err || { echo "timing of $lib failed ($?)"; exit 1; }
  cat $D/wl1_$lib.time
  echo "== $lib: counters" | tee -a $D/wl1_progress.log
  rm -rf $D/wl1_$lib
  timeout -k 10 300 rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_CACHE_MISS -d $D/wl1_$lib -o p -- $CMD > $D/wl1_$lib.json 2> $D/wl1_$lib.err || { echo "counter pass of $lib failed ($?)"; exit 1; }
done
python3 $R/tools/walk_l1_counters.py $D $OUT $W $K "$@"
for lib in "$@"; do rm -rf $D/wl1_$lib; done   # the counter databases are large
