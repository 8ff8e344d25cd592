"""What the tools/time_*.py scripts share: the package import, the config 3 scene and its two regimes, the sample statistics, the
device-event brackets, the copy yardstick, the body grid of the obstacle tools, the head and tail of a result file, and for the tools
of the spatial queries (time_neighbors, time_components, time_knn, time_rays, time_ray_spans, time_shell, time_aniso) the series of the engine's own brackets,
the queries through the C ABI alone, and the torch route a query is compared with."""
from __future__ import annotations

import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SPH_TREE", HERE)                                  # the tree the package is imported from (time_bodies.py's child processes)
sys.path.insert(0, ROOT)
pkg = importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd")

REPS = 25
REGIMES = (("lattice_state", 1), ("compressed", 300))


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
            "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)), "calls": int(len(us))}


def config3():
    """BASELINE.json configs[2]: 4 M particles, 128^3 cells.  Returns (config, records, params)."""
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    return cfg, rec, pkg.default_params(**syn.params_fields(cfg))


def regimes(f, plan=REGIMES, download=True, single_step_compute=False):
    """Advance engine f to each (label, substep) of the plan in turn and yield (label, substep, state): the downloaded records, or
    None with download=False.  single_step_compute: an advance by one substep is a DispatchCompute, not a DispatchN(1)."""
    done = 0
    for label, substep in plan:
        if substep - done == 1 and single_step_compute:
            f.DispatchCompute()
        elif substep > done:
            f.DispatchN(substep - done)
        done = substep
        f.sync()
        yield label, substep, f.download() if download else None


def other_us(f):
    """(microseconds, brackets) of the engine's timing class `other` since the last call."""
    ms, launches = f.kernel_times(reset=True)["other"]
    return ms * 1000.0, int(launches)


def other_per_dispatch(f, reps=REPS, warm=3):
    """Class `other` of each of `reps` single dispatches after `warm` warm-ups; leaves SPH_OPT_TIMING on.  One bracket per dispatch."""
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(warm):
        f.DispatchCompute()
    other_us(f)
    us = []
    for _ in range(reps):
        f.DispatchCompute()
        t, launches = other_us(f)
        assert launches == 1, launches
        us.append(t)
    return us


def events(fn, stream, reps=REPS, warm=3):
    """Device events on the stream around each of `reps` calls of fn after `warm` warm-ups."""
    import torch
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        us.append(a.elapsed_time(b) * 1000.0)
    return stats(us)


def series(f, fn, reps=REPS, warm=3, launches=None):
    """The engine's own brackets (SPH_OPT_TIMING) of each of `reps` calls of fn after `warm` warm-ups: (stats of class `other`, stats of
    the grid build's classes bin + scan + scatter).  A list given as `launches` receives the number of `other` brackets of each call."""
    for _ in range(warm):
        fn()
    f.kernel_times(reset=True)
    other, build = [], []
    for _ in range(reps):
        fn()
        t = f.kernel_times(reset=True)
        other.append(t["other"][0] * 1000.0)
        build.append(sum(t[c][0] for c in ("bin", "scan", "scatter")) * 1000.0)
        if launches is not None:
            launches.append(int(t["other"][1]))
    return stats(other), stats(build)


def _bare(f, fn, info, *args):
    """A query through the C ABI alone, without the copy of the result that the binding's method makes; returns the filled info."""
    pkg.engine._check(fn(f._h, *args, C.byref(info)))
    return info


def neighbors_build(f, R, flags=0):
    return _bare(f, f._L.sph_neighbors_build, pkg.SphNeighborInfo(), float(R), int(flags), 0)


def neighbors_query_count(f, pts, R):
    return _bare(f, f._L.sph_neighbors_query, pkg.SphNeighborInfo(), C.c_void_p(pts.data_ptr()), int(pts.shape[0]), float(R), pkg.SPH_NEIGHBORS_COUNT_ONLY, 0)


def components_build(f, R):
    return _bare(f, f._L.sph_components_build, pkg.SphComponentInfo(), float(R), pkg.SPH_COMPONENTS_FLUID_ONLY)


def knn_build(f, k, R):
    return _bare(f, f._L.sph_knn_build, pkg.SphKnnInfo(), int(k), float(R), 0)


def knn_query(f, pts, k, R):
    return _bare(f, f._L.sph_knn_query, pkg.SphKnnInfo(), C.c_void_p(pts.data_ptr()), int(pts.shape[0]), int(k), float(R), 0)


def rays_cast(f, dev, radius, flags):
    return _bare(f, f._L.sph_rays_cast_device, pkg.SphRaysInfo(), C.c_void_p(dev.data_ptr()), int(dev.shape[0]), float(radius), int(flags))


def rays_span(f, dev, radius, flags=0):
    return _bare(f, f._L.sph_rays_span_device, pkg.SphRaySpansInfo(), C.c_void_p(dev.data_ptr()), int(dev.shape[0]), float(radius), int(flags))


def shell_build(f, R):
    cfg = pkg.shell_config(radius=float(R))
    return _bare(f, f._L.sph_shell_build, pkg.SphShellInfo(), C.byref(cfg))


def aniso_build(f, R):
    cfg = pkg.aniso_config(radius=float(R))
    return _bare(f, f._L.sph_aniso_build, pkg.SphAnisoInfo(), C.byref(cfg))


def torch_route(route, compare, stream, reps):
    """What a query replaces, written in torch: device events on the torch stream around `reps` runs of route() after one warm-up, then
    compare(route()), a dict of what the comparison with the engine's result found.  Returns the stats with that dict, or, where the
    route does not fit (out of device memory, a tensor above a size limit such as torch.sort's INT_MAX elements), {"not_measured": the
    error's first line}; the cache is emptied either way."""
    import torch
    try:
        with torch.cuda.stream(stream):
            t = events(route, stream, reps=reps, warm=1)
            out = dict(t, **compare(route()))
    except RuntimeError as err:
        out = {"not_measured": str(err).splitlines()[0][:200]}
    torch.cuda.empty_cache()
    return out


def copy_yardstick(n, stream):
    """A device-to-device copy of arrays of the size of the engine's pos + vel state (two float4 per particle)."""
    import torch
    src = [torch.ones((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    dst = [torch.empty((n, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    with torch.cuda.stream(stream):
        for k in range(3 + REPS):
            a.record(stream)
            dst[0].copy_(src[0])
            dst[1].copy_(src[1])
            b.record(stream)
            b.synchronize()
            if k >= 3:
                us.append(a.elapsed_time(b) * 1000.0)
    return stats(us)


def body_grid(state, K):
    """K cells of a grid inside the fluid's bounding box: (centres, r) with r = 0.3 of a cell's smallest side."""
    fluid = state["pos"][state["isGhost"] == 0][:, :3].astype(np.float64)
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    side = int(np.ceil(K ** (1.0 / 3.0) - 1e-9))
    cell = (hi - lo) / side
    centres = [lo + cell * (np.array([k % side, (k // side) % side, k // (side * side)]) + 0.5) for k in range(K)]
    return centres, 0.3 * float(cell.min())


def moved_fraction(state, sp, stream, with_bodies):
    """Share of the records whose position differs after one substep on the engine with_bodies from one on a plain engine."""
    a, b = with_bodies, pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)
    a.DispatchCompute()
    b.DispatchCompute()
    ra, rb = a.download(), b.download()
    a.close()
    b.close()
    return float((ra["pos"] != rb["pos"]).any(axis=1).mean())


def out_path(args, feature):
    """The first argument, or time_<feature>.json in the current directory (the committed records in profiles/ are not overwritten)."""
    return args[0] if args else f"time_{feature}.json"


def header(tool, cfg, rec, variant_library=False, **extra):
    import torch
    head = {"tool": tool, "csrc_hash": pkg.build.csrc_hash()}
    if variant_library:
        head["library"] = os.path.basename(os.environ.get("SPH_HIP_LIB") or "libsph_hip.so")
    return dict(head, config=cfg.name, particles=int(len(rec)), device=torch.cuda.get_device_name(0), **extra)


def write_json(res, path, note=""):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", path, *([note] if note else []))
