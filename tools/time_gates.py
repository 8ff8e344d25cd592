"""Timing of the flow gates (include/sph_abi.h "flow gates") at config 3 (4 M particles, 128^3 cells), on the
lattice state (substep 1) and after 300 substeps (the compressed regime), with 1 and 8 gates, without scalars and
with K = 4 channels:

  gate_step       the gate step's own time per substep (k_gates<K> + k_gates_finish): the engine's device events (SPH_OPT_TIMING, class
                  `other`) of single dispatches with gates minus those of the same dispatches without them (with K = 4 the class also
                  holds the scalar step, one bracket)
  couple_sources8 the same difference for k_scalar_couple<4, true, false> + k_scalar_couple_finish with 8 world-frame sources: the
                  sweep the gate step is shaped after
  copy_yardstick  timing.copy_yardstick(n): a device-to-device copy of two float4 per particle (32 bytes read, 32 written); the gate
                  step reads pos[s] and sPV[2 s], 32 bytes per slot, plus vel and values of the crossers
  1 gate: an unbounded horizontal plane at the fluid's mid height.  8 gates: that plane, a gate_box of a quarter of the fluid's extent
  around its centre and an ellipse.

Device events on the engine's stream, warm-up, median and p10-p90 of the samples (run-to-run spread: p10-p90).
  python tools/time_gates.py [out.json]          (SPH_HIP_LIB selects a variant library, tools/build_variant.sh)
Without an argument the result goes to time_gates.json in the current directory; profiles/r25_time_gates.json is the committed record
of the first measurement.
"""
from __future__ import annotations

import json
import sys

import numpy as np

import timing
from timing import REPS, pkg, stats

F = np.float32


def gates_for(count, state):
    fluid = state["pos"][state["isGhost"] == 0][:, :3].astype(np.float64)
    lo, hi = fluid.min(axis=0), fluid.max(axis=0)
    c, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    plane = pkg.gate(pkg.SPH_GATE_RECT, c, (0, 0, 1), (1, 0, 0), unbounded=True)
    if count == 1:
        return [plane]
    return [plane, *pkg.gate_box(c, half), pkg.gate(pkg.SPH_GATE_ELLIPSE, c + np.array([0.0, 0.5 * half[1], 0.0]), (0, 0, half[2]), (half[0], 0, 0))]


def sources8(state):
    centres, r = timing.body_grid(state, 8)
    return [pkg.scalar_source(pkg.SPH_SOURCE_SPHERE if i % 2 else pkg.SPH_SOURCE_BOX, centres[i], 1.2 * r, channel=i % 4, rate=2.0) for i in range(8)]


def other_per_dispatch(e, reps=REPS, warm=3):
    """Class `other` of each of `reps` single dispatches after `warm` warm-ups: the scalar step, the coupling step and the gate step,
    one bracket each where they are on (0 where none is).  Leaves SPH_OPT_TIMING on."""
    e.set_option(pkg.SPH_OPT_TIMING, 1)
    for _ in range(warm):
        e.DispatchCompute()
    timing.other_us(e)
    us = []
    for _ in range(reps):
        e.DispatchCompute()
        us.append(timing.other_us(e)[0])
    return us


def main() -> None:
    import torch
    out_path = timing.out_path(sys.argv[1:], "gates")
    cfg, rec, sp = timing.config3()
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    res = timing.header("tools/time_gates.py", cfg, rec, variant_library=True, samples_per_case=REPS, regimes={})
    rng = np.random.default_rng(7)
    n = len(rec)
    copy = timing.copy_yardstick(n, stream)
    res["copy_yardstick"] = dict(copy, bytes_per_particle_moved=64)
    for label, substep, state in timing.regimes(f):
        r = {}
        for K in (0, 4):
            values = rng.random((n, K)).astype(F) if K else None
            other, crossings = {}, {}
            cases = ["none", "gates1", "gates8"] + (["sources8"] if K else [])
            for name in cases:
                e = pkg.SPHFluidGPU.from_particles(state, sp, stream=stream.cuda_stream)           # every case starts from the same state
                if K:
                    e.set_scalars(values, diffusivity=0.0)
                if name.startswith("gates"):
                    e.set_gates(gates_for(int(name[5:]), state))
                if name == "sources8":
                    e.set_scalar_sources(sources8(state))
                other[name] = stats(other_per_dispatch(e))
                if name.startswith("gates"):
                    rows, _, steps = e.gate_books()
                    crossings[name] = [float(x) / max(steps, 1) for x in (rows["forward"] + rows["backward"])]
                e.close()
            step = {name: other[name]["median_us"] - other["none"]["median_us"] for name in cases[1:]}
            r[f"K{K}"] = {"class_other_per_dispatch": other, "step_us": step, "crossings_per_substep": crossings,
                          "over_copy": {name: step[name] / copy["median_us"] for name in step},
                          "gates8_over_gates1": step["gates8"] / step["gates1"],
                          **({"gates_over_couple_sources8": {g: step[g] / step["sources8"] for g in ("gates1", "gates8")}} if K else {})}
            print(label, K, json.dumps({"step_us": step, "copy_us": copy["median_us"]}), flush=True)
        res["regimes"][label] = dict(substep=substep, **r)
    f.close()
    timing.write_json(res, out_path)


if __name__ == "__main__":
    main()
