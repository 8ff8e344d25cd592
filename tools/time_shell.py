"""Timing of the free-surface shell (include/sph_abi.h "free-surface particles") at config 3 (4 M particles, 128^3 cells, h = cellSize)
after 300 substeps (the compressed regime), at R = h and R = 2h.

A build synchronises, so device events around a call would time the host as well.  The numbers are the engine's own brackets
(SPH_OPT_TIMING, class `other`), one series per case after warm-ups, all in ONE process on ONE state.  SPH_OPT_SHELL_TIMED picks which
launches of a build the bracket covers; the launches themselves are the same:

  shell[R].whole          ids, k_shell_gather, the scan and compaction of ids[], the scan and compaction of the shell slots, k_shell_crest
  shell[R].pass1          ids + k_shell_gather                       (SPH_OPT_SHELL_TIMED 1)
  shell[R].pass2          k_shell_crest                              (SPH_OPT_SHELL_TIMED 2); pass2_ns_per_shell_particle = median / numShell
  shell[R].compactions    the two scans (three kernels each) and the two k_shell_compact launches        (SPH_OPT_SHELL_TIMED 3)
  count_walk[R]           sph_neighbors_build with SPH_NEIGHBORS_COUNT_ONLY at the same R, in the same run: ids, k_neighbors_count and the
                          scan of the counts -- the plain walk over the same candidates that writes 4 bytes per target; the yardstick.
                          pass1_over_count_walk and whole_over_count_walk are the ratios of the medians
  torch_route[R=h]        what pass 1 replaces: radius_graph(R), a gather of the positions, w = (R^2 - r^2)^2 per edge and three
                          index_add_ (W, S) -- atomic sums, not reproducible; device events on the torch stream around the whole route
                          (it includes the list build and its export).  Where it does not fit, the file says so
  grid_build              bin + scan + scatter classes of the same calls (what every build runs first)

  python tools/time_shell.py [out.json]
Without an argument the result goes to time_shell.json in the current directory; profiles/r19_time_shell.json is the committed record.
"""
from __future__ import annotations

import json
import sys

import timing
from timing import pkg, series, shell_build as shell

SLOW_REPS = 3                                                                    # runs of the torch route


def torch_route(f, pos, R):
    """W and S of pass 1 from the radius graph in torch: (W (n,), S (n, 3))."""
    import torch
    g = f.radius_graph(R)
    recv, send = g[0], g[1]
    d = pos[send] - pos[recv]
    t = R * R - (d * d).sum(dim=1)
    w = t * t
    n = pos.shape[0]
    W = torch.zeros(n, dtype=torch.float32, device=pos.device).index_add_(0, recv, w)
    S = torch.zeros((n, 3), dtype=torch.float32, device=pos.device).index_add_(0, recv, w[:, None] * d)
    return W, S


def main() -> None:
    import numpy as np
    import torch
    out_path = timing.out_path(sys.argv[1:], "shell")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    n = len(rec)
    h = sp.param_h
    res = timing.header("tools/time_shell.py", cfg, rec, reps=timing.REPS, slow_reps=SLOW_REPS, regimes={})
    for label, substep, state in timing.regimes(f, (("compressed", 300),)):
        pos = torch.from_numpy(np.ascontiguousarray(state["pos"][:, :3])).cuda()
        r = {}
        for name, R in (("R=h", h), ("R=2h", 2.0 * h)):
            v = {}
            walk, grid_us = series(f, lambda: timing.neighbors_build(f, R, pkg.SPH_NEIGHBORS_COUNT_ONLY))
            ni = f.neighbor_info()
            v["count_walk"] = dict(walk, total=int(ni.total), mean_degree=ni.total / n, max_count=int(ni.maxCount))
            v["grid_build"] = grid_us
            sh = {}
            for part, key in ((0, "whole"), (1, "pass1"), (2, "pass2"), (3, "compactions")):
                f.set_option(pkg.SPH_OPT_SHELL_TIMED, part)
                sh[key], _ = series(f, lambda: shell(f, R))
            f.set_option(pkg.SPH_OPT_SHELL_TIMED, 0)
            si = f.shell_info()
            sh["info"] = dict(rows=int(si.rows), num_shell=int(si.numShell), shell_share=si.numShell / n, num_isolated=int(si.numIsolated),
                              max_count=int(si.maxCount), stencil=int(si.stencil))
            sh["pass1_over_count_walk"] = sh["pass1"]["median_us"] / walk["median_us"]
            sh["whole_over_count_walk"] = sh["whole"]["median_us"] / walk["median_us"]
            sh["pass2_ns_per_shell_particle"] = 1000.0 * sh["pass2"]["median_us"] / max(1, int(si.numShell))
            sh["pass1_ns_per_accepted_pair"] = 1000.0 * sh["pass1"]["median_us"] / max(1, int(ni.total))
            v["shell"] = sh
            print(label, name, json.dumps({k: sh[k]["median_us"] for k in ("whole", "pass1", "pass2", "compactions")}), "count walk", walk["median_us"],
                  "shell", si.numShell, flush=True)
            if name == "R=h":
                # the torch route once (pass 1 only); checked against the engine's rows through the offset ratio where W > 0
                def offset_ratios(routed):
                    W, S = routed
                    z = f.shell(R, device=True)[0]
                    stream.synchronize()
                    ratio = torch.where(W > 0, S.norm(dim=1) / (float(R) * W.clamp_min(1e-30)), torch.zeros_like(W))
                    return dict(edges=int(ni.total), max_offset_ratio_difference=float((ratio - z[:, 3]).abs().max()))
                v["torch_route_pass1"] = route = timing.torch_route(lambda: torch_route(f, pos, float(np.float32(R))), offset_ratios, stream, SLOW_REPS)
                if "not_measured" not in route:
                    v["torch_route_over_pass1"] = route["median_us"] / sh["pass1"]["median_us"]
                print(label, name, "torch route", json.dumps(v["torch_route_pass1"]), flush=True)
            r[name] = v
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
