"""Timing of the field sampler (include/sph_abi.h "field sampling") at config 3 (4 M particles, 128^3 cells, h = cellSize), on the
lattice state (substep 0) and after 300 substeps (the compressed regime):

  (a) a 256^3 lattice over the grid at spacing h/2, SPH_FIELD_DENSITY   (k_sample_lattice: LDS-staged bricks)
  (b) the same lattice, SPH_FIELD_ALL
  (c) (a)'s points through sph_sample_points_device                     (k_sample_points: the plain kernel; same bits as (b))
  (d) 1 M random probes inside the grid
  (e) the grid build every call runs first (a call with m = 0)

Device events on the engine's stream around each call, 3 warm-up calls, median and spread of 25.
  python tools/time_sample.py [out.json]
Without an argument the result goes to time_sample.json in the current directory; profiles/r06_time_sample.json is the committed
record of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import pkg


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "sample")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    g = f.ComputeGridExtents()
    h = sp.param_h
    spacing = (h / 2, h / 2, h / 2)
    dims = (2 * g.dims[0], 2 * g.dims[1], 2 * g.dims[2])
    npts = dims[0] * dims[1] * dims[2]
    origin = tuple(float(x) for x in g.gridMin)
    axes = [torch.tensor(np.float32(origin[a]) + np.arange(dims[a], dtype=np.float32) * np.float32(spacing[a]), device="cuda") for a in range(3)]
    Z, Y, X = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    lat_pts = torch.zeros((npts, 4), dtype=torch.float32, device="cuda")
    lat_pts[:, 0], lat_pts[:, 1], lat_pts[:, 2] = X.reshape(-1), Y.reshape(-1), Z.reshape(-1)
    del X, Y, Z
    rng = np.random.default_rng(7)
    lo = np.array(g.gridMin, np.float32)
    hi = lo + np.float32(g.cellSize) * np.array(g.dims, np.float32)
    rnd = np.zeros((1 << 20, 4), np.float32)
    rnd[:, :3] = lo + (hi - lo) * rng.random((1 << 20, 3))
    rnd_pts = torch.from_numpy(rnd).cuda()
    out_f = torch.empty(npts, dtype=torch.float32, device="cuda")
    out_all = torch.empty((npts, 8), dtype=torch.float32, device="cuda")
    out_pts = torch.empty((npts, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        return timing.events(fn, stream)

    res = timing.header("tools/time_sample.py", cfg, rec, grid=list(g.dims), lattice=list(dims), lattice_points=int(npts), spacing="h/2",
                        random_probes=1 << 20, regimes={})
    for label, substep, _ in timing.regimes(f, (("lattice_state", 0), ("compressed", 300)), download=False):
        r = {}
        r["a_lattice_density"] = timed(lambda: f.sample_lattice_device(origin, spacing, dims, out_f.data_ptr(), pkg.SPH_FIELD_DENSITY))
        r["b_lattice_all"] = timed(lambda: f.sample_lattice_device(origin, spacing, dims, out_all.data_ptr(), pkg.SPH_FIELD_ALL))
        r["c_points_plain_kernel"] = timed(lambda: f.sample_device(lat_pts.data_ptr(), npts, out_pts.data_ptr()))
        r["d_random_probes_1M"] = timed(lambda: f.sample_device(rnd_pts.data_ptr(), 1 << 20, out_pts.data_ptr()))
        r["e_grid_build"] = timed(lambda: f.sample_device(0, 0, 0))
        # the plain-kernel A/B must return the same bits as the staged lattice
        f.sample_lattice_device(origin, spacing, dims, out_all.data_ptr(), pkg.SPH_FIELD_ALL)
        f.sample_lattice_device(origin, spacing, dims, out_f.data_ptr(), pkg.SPH_FIELD_DENSITY)
        f.sample_device(lat_pts.data_ptr(), npts, out_pts.data_ptr())
        f.sync()
        r["c_equals_b_bitwise"] = bool(torch.equal(out_all.view(torch.int32), out_pts.view(torch.int32)))
        r["a_equals_c_density_bitwise"] = bool(torch.equal(out_f.view(torch.int32), out_pts[:, 0].contiguous().view(torch.int32)))
        cnt = out_pts[:, 3].contiguous().view(torch.int32)
        r["mean_neighbours_within_h"] = float(cnt.double().mean())
        b = r["e_grid_build"]["median_us"]
        for k in ("a_lattice_density", "b_lattice_all", "c_points_plain_kernel", "d_random_probes_1M"):
            r[k]["build_share"] = b / r[k]["median_us"]
        res["regimes"][label] = dict(substep=substep, **r)
        print(label, json.dumps({k: (v["median_us"] if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
