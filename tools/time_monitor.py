"""Timing of the field monitors (include/sph_abi.h "field monitors") at config 3 (4 M particles, 128^3 cells), on
the lattice state (substep 1) and after 300 substeps (the compressed regime):

  points4096        the monitor step's own time per substep (k_monitor_points + k_monitor_tick) of an explicit monitor of 4096 points
                    spread over the fluid's bounding box, every 1: the engine's device events (SPH_OPT_TIMING, class `other`; without
                    a monitor a plain dispatch has no bracket of that class) of single dispatches
  lattice128_every1 the same for a lattice monitor of 128^3 points over the fluid's bounding box (k_monitor_lattice + k_monitor_tick)
  lattice128_every8 the same lattice with every 8: the acting dispatches (one in eight) and the others apart
  idle_launch       the non-acting dispatches of lattice128_every8: a launch of up to 2^20 blocks that read one word and return, and the tick
  sampler_all       sph_sample_lattice(SPH_FIELD_ALL) on the same lattice in the same process (class `other` of the call; its grid build
                    is timed under the grid build's classes and is not part of it): the kernel the monitor's is built from
  copy_yardstick    timing.copy_yardstick(n): a device-to-device copy of two float4 per particle, for the bandwidth the estimate uses
  estimate          sampler_all + the row traffic at the yardstick's bandwidth, 256 bytes per point (a 128-byte row read and written),
                    less the 32 bytes per point the sampler stores and the monitor does not; measured_over_estimate is the ratio to it

Device events on the engine's stream, warm-up, median and p10-p90 of the samples (run-to-run spread: p10-p90).
  python tools/time_monitor.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_monitor.json in the current directory; profiles/r26_time_monitor.json is the committed record
of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import REPS, pkg, stats

F = np.float32
DIMS = (128, 128, 128)


def fluid_box(state):
    fluid = state["pos"][state["isGhost"] == 0][:, :3].astype(np.float64)
    return fluid.min(axis=0), fluid.max(axis=0)


def per_dispatch(e, reps, warm):
    """Class `other` of each of `reps` single dispatches after `warm` warm-ups (one bracket per monitor slot).  Leaves SPH_OPT_TIMING on."""
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(warm):
        e.DispatchCompute()
    timing.other_us(e)
    us = []
    for _ in range(reps):
        e.DispatchCompute()
        t, brackets = timing.other_us(e)
        assert brackets == 1, brackets
        us.append(t)
    return us


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "monitor")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    res = timing.header("tools/time_monitor.py", cfg, rec, variant_library=True, samples_per_case=REPS, regimes={})
    n = len(rec)
    copy = timing.copy_yardstick(n, stream)
    res["copy_yardstick"] = dict(copy, bytes_per_particle_moved=64)
    bytes_per_us = 64.0 * n / copy["median_us"]
    points = int(np.prod(DIMS))
    rng = np.random.default_rng(7)
    for label, substep, state in timing.regimes(f):
        lo, hi = fluid_box(state)
        spacing = ((hi - lo) / (np.array(DIMS) - 1)).astype(F)
        origin = lo.astype(F)
        r = {"lattice": dict(origin=origin.tolist(), spacing=spacing.tolist(), dims=list(DIMS), spacing_over_h=(spacing / F(sp.param_h)).tolist())}

        def fresh():
            return pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)               # every case starts from the same state
        e = fresh()
        e.set_monitor((lo + rng.random((4096, 3)) * (hi - lo)).astype(F))
        r["points4096"] = stats(per_dispatch(e, REPS, 3))
        e.close()
        e = fresh()
        e.set_monitor(lattice=(origin, spacing, DIMS))
        r["lattice128_every1"] = stats(per_dispatch(e, REPS, 3))
        wet = e.monitor_rows()["wet"]
        r["lattice_wet_share_of_points"] = float((wet > 0).mean())
        e.close()
        e = fresh()
        e.set_monitor(lattice=(origin, spacing, DIMS), every=8)
        us = np.array(per_dispatch(e, 8 * 12, 8))                                                       # (the warm-up is one whole period: sample 0 acts)
        r["lattice128_every8"] = dict(acting=stats(us[0::8]), all=stats(us), mean_us_per_substep=float(us.mean()))
        r["idle_launch"] = stats(us[np.arange(len(us)) % 8 != 0])
        assert e.monitor_info()["acting"] == 13, e.monitor_info()
        e.close()
        e = fresh()
        buf = torch.empty(points * 8, dtype=torch.float32, device="cuda")
        e.set_option(pkg.SPH_OPT_TIMING, 1)
        r["sampler_all"] = timing.series(e, lambda: e.sample_lattice_device(origin, spacing, DIMS, buf.data_ptr(), pkg.SPH_FIELD_ALL))[0]
        e.close()
        del buf
        rows_us = (256.0 - 32.0) * points / bytes_per_us
        estimate = r["sampler_all"]["median_us"] + rows_us
        r["estimate"] = dict(row_traffic_us=rows_us, us=estimate, bytes_per_us=bytes_per_us,
                             measured_over_estimate=r["lattice128_every1"]["median_us"] / estimate,
                             measured_over_sampler=r["lattice128_every1"]["median_us"] / r["sampler_all"]["median_us"],
                             estimate_over_sampler=estimate / r["sampler_all"]["median_us"])
        print(label, json.dumps({k: (v.get("median_us", v) if isinstance(v, dict) else v) for k, v in r.items() if k != "lattice"}), flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
