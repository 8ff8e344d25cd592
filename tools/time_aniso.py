"""Timing of the anisotropic kernels (include/sph_abi.h "anisotropic kernels") at config 3 (4 M particles, 128^3 cells, h = cellSize)
after 300 substeps (the compressed regime), at the default config (R = 2h, support h).

A build synchronises, so device events around a call would time the host as well.  The numbers are the engine's own brackets
(SPH_OPT_TIMING, class `other`), one series per case after warm-ups, all in ONE process on ONE state:

  gather                  sph_aniso_build: ids + k_aniso_gather
  shell_pass1             sph_shell_build at the same R with SPH_OPT_SHELL_TIMED 1: ids + k_shell_gather -- the same walk over the same
                          candidates with five sums in place of eleven and no eigen-decomposition; gather_over_shell_pass1 is the ratio
                          of the medians
  lattice_whole           sph_aniso_lattice on the lattice of spacing h/2 over the grid box: ids + k_aniso_gather + k_aniso_lattice;
                          lattice_kernel_us = its median less the median of `gather` (k_aniso_lattice alone, derived)
  sample_lattice          sph_sample_lattice (SPH_FIELD_FRACTION) on the same lattice: k_sample_lattice, the staged isotropic sampler;
                          lattice_over_sample_lattice is lattice_kernel_us over its median
  aniso_surface / surface sph_aniso_surface beside sph_extract_surface (SPH_FIELD_FRACTION) on that lattice at iso 0.5: the field and the
                          four launches of the mesher each; the vertex and triangle counts of both
  info                    reachStencil, numSparse, numClamped, maxCount, maxReach of the build
  grid_build              bin + scan + scatter classes of the same calls (what every build runs first)

  python tools/time_aniso.py [out.json]
Without an argument the result goes to time_aniso.json in the current directory; profiles/r21_time_aniso.json is the committed record.
The tool has no pass or fail threshold."""
from __future__ import annotations

import ctypes as C
import json
import sys

import timing
from timing import pkg, series


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "aniso")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    n = len(rec)
    h = sp.param_h
    R = 2.0 * h
    res = timing.header("tools/time_aniso.py", cfg, rec, reps=timing.REPS, regimes={})
    eng = pkg.engine
    for label, substep, _ in timing.regimes(f, (("compressed", 300),), download=False):
        v = {}
        g = f.ComputeGridExtents()
        s = 0.5 * h
        origin = tuple(float(x) for x in g.gridMin)
        dims = tuple(int(round(g.cellSize * d / s)) for d in g.dims)
        nodes = dims[0] * dims[1] * dims[2]
        v["lattice"] = dict(origin=origin, spacing=s, dims=dims, nodes=nodes)
        buf = torch.empty(nodes, dtype=torch.float32, device="cuda")
        acfg = pkg.aniso_config()
        o3, s3, d3 = eng._f3(origin), eng._f3((s, s, s)), eng._dims3(dims)

        v["gather"], v["grid_build"] = series(f, lambda: timing.aniso_build(f, R))
        ai = f.aniso_info()
        v["info"] = dict(rows=int(ai.rows), num_sparse=int(ai.numSparse), num_clamped=int(ai.numClamped), max_count=int(ai.maxCount),
                         max_reach_over_h=float(ai.maxReach) / h, stencil=int(ai.stencil), reach_stencil=int(ai.reachStencil))
        f.set_option(pkg.SPH_OPT_SHELL_TIMED, 1)
        v["shell_pass1"], _ = series(f, lambda: timing.shell_build(f, R))
        f.set_option(pkg.SPH_OPT_SHELL_TIMED, 0)
        v["gather_over_shell_pass1"] = v["gather"]["median_us"] / v["shell_pass1"]["median_us"]
        v["gather_ns_per_particle"] = 1000.0 * v["gather"]["median_us"] / n
        print(label, "gather", v["gather"]["median_us"], "shell pass 1", v["shell_pass1"]["median_us"], json.dumps(v["info"]), flush=True)

        def aniso_lattice():
            info = pkg.SphAnisoInfo()
            eng._check(f._L.sph_aniso_lattice(f._h, C.byref(acfg), o3, s3, d3, C.c_void_p(buf.data_ptr()), C.byref(info)))
        v["lattice_whole"], _ = series(f, aniso_lattice)
        v["lattice_kernel_us"] = v["lattice_whole"]["median_us"] - v["gather"]["median_us"]
        v["sample_lattice"], _ = series(f, lambda: f.sample_lattice_device(origin, (s, s, s), dims, buf.data_ptr(), pkg.SPH_FIELD_FRACTION))
        v["lattice_over_sample_lattice"] = v["lattice_kernel_us"] / v["sample_lattice"]["median_us"]
        v["lattice_ns_per_node"] = 1000.0 * v["lattice_kernel_us"] / nodes
        print(label, "aniso lattice", v["lattice_whole"]["median_us"], "kernel", v["lattice_kernel_us"], "sample lattice", v["sample_lattice"]["median_us"], flush=True)

        surf = pkg.SphSurface()

        def aniso_surface():
            info = pkg.SphAnisoInfo()
            eng._check(f._L.sph_aniso_surface(f._h, C.byref(acfg), o3, s3, d3, 0.5, C.byref(surf), C.byref(info)))
        v["aniso_surface"], _ = series(f, aniso_surface)
        v["aniso_surface"].update(vertices=int(surf.numVertices), triangles=int(surf.numTriangles))
        v["surface"], _ = series(f, lambda: f.extract_surface(origin, (s, s, s), dims, 0.5, pkg.SPH_FIELD_FRACTION))
        iso = f.extract_surface(origin, (s, s, s), dims, 0.5, pkg.SPH_FIELD_FRACTION)
        v["surface"].update(vertices=int(iso.numVertices), triangles=int(iso.numTriangles))
        v["aniso_surface_over_surface"] = v["aniso_surface"]["median_us"] / v["surface"]["median_us"]
        print(label, "aniso surface", v["aniso_surface"]["median_us"], "surface", v["surface"]["median_us"], flush=True)
        res["regimes"][label] = dict(substep=substep, **v)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
