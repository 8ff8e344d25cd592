"""Seeded random scenes (support.random_scene: kernel lengths, grids down to three cells, clumps, ghosts, particles outside the grid,
every container shape; at most 2000 records) after a few dispatches: the device's ray spans are sph_rays_span_host's bytes on the
downloaded records, with the radius in (0, cellSize / 2], fluid_only, the span walk, the order of the rays and the rays (void ones
among them) drawn from the seed.  Every launch is bounded by the number of rays and the walk by the grid's size."""
import numpy as np
import pytest

import ray_spans_ref as SR
import rays_scenes as RS
from support import random_scene, same_info

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_random_scene(pkg, seed):
    rec, sp, steps, what = random_scene(pkg, seed)
    if len(rec) > 2000:
        rec = rec[:2000].copy()
    rng = np.random.default_rng(9100 + seed)
    g = pkg.compute_grid_extents(sp)
    cs = F(g.cellSize)
    radius = float(F(rng.choice([0.5, 0.5, rng.uniform(0.01, 0.5), rng.uniform(0.01, 0.5), 0.25, 0.02])) * cs)
    fluid_only = bool(rng.integers(2))
    walk, order = int(rng.integers(2)), int(rng.integers(2))
    print(what, "radius", radius, "fluid_only", fluid_only, "walk", walk, "order", order)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, walk)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, order)
    for _ in range(2):
        f.DispatchN(steps)
    now = f.download()
    lo, ext = np.array(list(g.gridMin), F), np.array(list(g.dims), F) * cs
    m = 2011                                                                       # no multiple of 64
    o = lo + (rng.random((m, 3)).astype(F) * F(2.0) - F(0.5)) * ext                # inside and outside the grid's box
    target = lo + rng.random((m, 3)).astype(F) * ext
    r = RS.rays(o, target - o, 0.0, np.inf)
    r[: m // 3, 7] = F(0.2) + rng.random(m // 3).astype(F) * F(1.5)                # a third are segments
    r[m // 3: m // 2, 3] = F(-0.5)                                                 # some start behind the origin
    axis = rng.integers(3, size=m)
    zero = rng.random(m) < 0.2                                                     # a fifth have a zero direction component
    r[np.flatnonzero(zero), 4 + axis[zero]] = 0
    r = RS.void_mix(r, rng, share=0.05)
    want, info = pkg.ray_spans_host(now, sp, r, radius, fluid_only=fluid_only, with_info=True)
    SR.same_rows(f.ray_spans(r, radius, fluid_only=fluid_only), want, str(what))
    same_info(f.ray_spans_info(), info, SR.INFO_FIELDS, str(what))
    assert info.voidRays > 0
    # the host's copy of both walks, and the other walk, order and flag on the same state
    for variant in (0, 1):
        SR.same_rows(pkg.ray_spans_walk_host(now, sp, r, radius, fluid_only=fluid_only, variant=variant), want, f"{what} (walk {variant} on the host)")
    f.set_option(pkg.SPH_OPT_RAY_SPANS_VARIANT, 1 - walk)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 1 - order)
    SR.same_rows(f.ray_spans(r, radius, fluid_only=not fluid_only), pkg.ray_spans_host(now, sp, r, radius, fluid_only=not fluid_only), f"{what} the other walk")
    f.close()
