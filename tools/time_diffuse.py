"""Timing of the secondary particles (include/sph_abi.h "spray, foam and bubbles") at config 3 (4 M particles,
128^3 cells), on the lattice state (substep 0, after the one substep that gives the records a density) and after 300 substeps (the
compressed regime), with a pool of C = 1 048 576 records:

  advance       k_diffuse_advance alone with a full pool (records seeded uniformly in the fluid's bounding box, nothing spawns, nothing
                dies of life or age): the engine's own device events around that launch (SPH_OPT_TIMING with SPH_OPT_DIFFUSE_TIMED 1,
                class `other`), one sample per dispatch; once with the records in random order and once with the same records sorted
                by the cell they start in (the pool keeps its order while nothing dies), which is the order k_tracer_advect gives
                itself through perm[]
  yardstick     k_tracer_advect<false> + k_tracer_tick for as many tracers seeded at the same positions, on a second engine started
                from the same state, in the same session (dispatches that also re-sort the processing order are left out)
  spawn_side    count over N, scan over N, scan over C, compaction, emit and tick (SPH_OPT_DIFFUSE_TIMED 2): once with the full pool
                of `advance` (all C records compacted, nothing born) and once under churn (every particle a parent with a small rate,
                every record dead after three substeps), with the bytes those launches must move and the bandwidth that makes,
                beside the same figures for k_bin and for k_scatter + k_rank of the same dispatches

Device events on the engine's stream, warm-up, median and p10-p90 of the samples.
  python tools/time_diffuse.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_diffuse.json in the current directory; profiles/r14_time_diffuse.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import other_us, pkg, stats

F = np.float32
C_POOL = 1 << 20


def seeds(state, m, rng):
    fluid = state["pos"][state["isGhost"] == 0][:, :3]
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    return (lo + (hi - lo) * rng.random((m, 3))).astype(F)


def class_us(f):
    """{class: (microseconds, brackets)} since the last call."""
    return {k: (ms * 1000.0, int(n)) for k, (ms, n) in f.kernel_times(reset=True).items()}


def bytes_moved(n, C, before, after):
    """What the spawn side of ONE substep must read and write, from the counts of that substep."""
    spawned = after["spawned"] - before["spawned"]
    born = spawned - (after["dropped"] - before["dropped"])
    survivors = after["alive"] - born
    count = n * (16 + 16 + 4)                 # own data, the 16 bytes of the sorted record that hold 1/rho, cnt[id]
    scan_n = n * (4 + 4 + 4 + 4)              # reduce reads, apply reads, writes the prefix and the zeros
    scan_c = C * (4 + 4 + 4 + 4)
    compact = before["alive"] * 8 + survivors * (48 + 48)
    emit = n * (16 + 8) + born * 48           # own data and two prefix words per slot, 48 bytes per newborn (the parents' records come on top)
    return dict(bytes=count + scan_n + scan_c + compact + emit, spawned=spawned, born=born, survivors=survivors)


def by_cell(pts, sp):
    g = pkg.compute_grid_extents(sp)
    c = [np.clip(np.floor((pts[:, a] - F(g.gridMin[a])) / F(g.cellSize)), 0, g.dims[a] - 1).astype(np.int64) for a in range(3)]
    return pts[np.argsort((c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0], kind="stable")]


def full_pool(state, sp, stream, pts, reps, modes=(("advance", 1), ("spawn_side", 2))):
    """advance and spawn side with a full pool that nothing enters or leaves (but for records that the flow carries out of the box)."""
    e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    cfg = pkg.diffuse_config(capacity=C_POOL, rate=0.0, maxAge=1e30, lifeMin=1e9, lifeMax=1e9)
    e.set_diffuse(cfg)
    rec = np.zeros(C_POOL, pkg.DIFFUSE_DTYPE)
    rec["pos"], rec["life"] = pts, 1e9
    e.seed_diffuse(rec)
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    out = {}
    for label, mode in modes:
        e.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, mode)
        for _ in range(3):
            e.DispatchCompute()
        class_us(e)
        us, side, bins, scat = [], [], [], []
        for _ in range(reps):
            before = e.diffuse_info()
            e.DispatchCompute()
            t = class_us(e)
            assert t["other"][1] == 1, t
            us.append(t["other"][0])
            bins.append(t["bin"][0])
            scat.append(t["scatter"][0])
            if mode == 2:
                side.append(bytes_moved(len(state), C_POOL, before, e.diffuse_info()))
        out[label] = stats(us)
        if mode == 2:
            out[label].update(bandwidth(side, us))
            n = len(state)
            out["k_bin"] = dict(stats(bins), bytes=n * 24, GBps=n * 24 / np.median(bins) / 1e3)
            out["k_scatter_and_k_rank"] = dict(stats(scat), bytes=n * 128, GBps=n * 128 / np.median(scat) / 1e3)
    info = e.diffuse_info()
    out["alive_at_the_end"] = info["alive"]
    out["kinds_at_the_end"] = info["aliveByKind"]
    e.close()
    return out


def bandwidth(side, us):
    b = float(np.median([s["bytes"] for s in side]))
    return dict(bytes=b, GBps=b / float(np.median(us)) / 1e3, born_per_substep=float(np.median([s["born"] for s in side])),
                survivors_per_substep=float(np.median([s["survivors"] for s in side])))


def churn(state, sp, stream, reps):
    """The spawn side while records are born and die: every particle is a parent (threshold below every foam factor), lambda = 0.05
    per substep at padA = 0, every record dies three substeps after its birth."""
    e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    dt = float(sp.param_timeStep)
    cfg = pkg.diffuse_config(capacity=C_POOL, threshold=-1.0, rate=0.05 / dt, maxAge=2.5 * dt, lifeMin=2.5 * dt, lifeMax=2.5 * dt, maxPerParent=2)
    e.set_diffuse(cfg)
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    e.set_option(pkg.SPH_OPT_DIFFUSE_TIMED, 2)
    for _ in range(6):
        e.DispatchCompute()
    class_us(e)
    us, side = [], []
    for _ in range(reps):
        before = e.diffuse_info()
        e.DispatchCompute()
        t = class_us(e)
        us.append(t["other"][0])
        side.append(bytes_moved(len(state), C_POOL, before, e.diffuse_info()))
    out = dict(stats(us), **bandwidth(side, us), alive_at_the_end=e.diffuse_info()["alive"])
    e.close()
    return out


def tracer_yardstick(state, sp, stream, pts, reps):
    e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    p4 = np.zeros((len(pts), 4), F)
    p4[:, :3] = pts
    e.set_tracers(p4, pkg.SPH_TRACER_EULER)
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(3):
        e.DispatchCompute()
    other_us(e)
    plain = []
    while len(plain) < reps:
        e.DispatchCompute()
        us, launches = other_us(e)
        if launches == 1:
            plain.append(us)
    e.close()
    return stats(plain)


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "diffuse")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    reps = timing.REPS
    res = timing.header("tools/time_diffuse.py", cfg, rec, variant_library=True, capacity=C_POOL, samples_per_case=reps, regimes={})
    rng = np.random.default_rng(7)
    for label, substep, state in timing.regimes(f):
        pts = seeds(state, C_POOL, rng)
        r = full_pool(state, sp, stream, pts, reps)
        r["advance_cell_order"] = full_pool(state, sp, stream, by_cell(pts, sp), reps, modes=(("advance", 1),))["advance"]
        r["yardstick_k_tracer_advect"] = tracer_yardstick(state, sp, stream, pts, reps)
        r["advance_over_yardstick"] = r["advance"]["median_us"] / r["yardstick_k_tracer_advect"]["median_us"]
        r["advance_cell_order_over_yardstick"] = r["advance_cell_order"]["median_us"] / r["yardstick_k_tracer_advect"]["median_us"]
        r["spawn_side_churn"] = churn(state, sp, stream, reps)
        res["regimes"][label] = dict(substep=substep, **r)
        print(label, json.dumps({k: (v["median_us"] if isinstance(v, dict) and "median_us" in v else v) for k, v in r.items()}), flush=True)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
