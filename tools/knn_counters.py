"""Driver for tools/knn_counters.sh: config 3 after 300 substeps, then `calls` calls each of sph_knn_build(k, R) with the default kernel
and of sph_neighbors_build(R), so that one rocprofv3 --pmc pass sees k_knn beside k_neighbors_count / k_neighbors_fill on one state.
  python tools/knn_counters.py [k] [R over h] [calls]"""
from __future__ import annotations

import sys

import timing
import time_knn


def main() -> None:
    import torch
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    fac = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = timing.pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.DispatchN(300)
    f.sync()
    for _ in range(calls):
        time_knn.knn(f, k, fac * sp.param_h)
        time_knn.lists(f, fac * sp.param_h)
    f.close()


if __name__ == "__main__":
    main()
