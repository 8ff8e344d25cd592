"""Seeded random scenes (support.random_scene: kernel lengths, grids down to three cells, clumps, ghosts, particles outside the grid,
every container shape) after a few dispatches: the device's ray hits are sph_rays_host's bytes on the downloaded records, with the
radius in (0, cellSize / 2], the flags, the order in which the rays are cast and the rays (void ones among them) drawn from the seed.  Every launch is bounded by the number of
rays and the walk by the grid's size."""
import numpy as np
import pytest

import rays_scenes as RS
from support import random_scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_random_scene(pkg, seed):
    rec, sp, steps, what = random_scene(pkg, seed)
    if len(rec) > 2000:
        rec = rec[:2000].copy()
    rng = np.random.default_rng(9000 + seed)
    g = pkg.compute_grid_extents(sp)
    cs = F(g.cellSize)
    radius = float(F(rng.choice([0.5, 0.5, rng.uniform(0.01, 0.5), rng.uniform(0.01, 0.5), 0.25, 0.02])) * cs)
    kw = dict(fluid_only=bool(rng.integers(2)), any_hit=bool(rng.integers(4) == 0))
    variant = int(rng.integers(2))
    print(what, "radius", radius, kw, "variant", variant)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, variant)
    for _ in range(2):
        f.DispatchN(steps)
    now = f.download()
    lo, ext = np.array(list(g.gridMin), F), np.array(list(g.dims), F) * cs
    m = 1531                                                                       # no multiple of 64
    o = lo + (rng.random((m, 3)).astype(F) * F(2.0) - F(0.5)) * ext                # inside and outside the grid's box
    target = lo + rng.random((m, 3)).astype(F) * ext
    r = RS.rays(o, target - o, 0.0, np.inf)
    r[: m // 3, 7] = F(0.2) + rng.random(m // 3).astype(F) * F(1.5)                # a third are segments
    r[m // 3: m // 2, 3] = F(-0.5)                                                 # some start behind the origin
    axis = rng.integers(3, size=m)
    zero = rng.random(m) < 0.2                                                     # a fifth have a zero direction component
    r[np.flatnonzero(zero), 4 + axis[zero]] = 0
    r = RS.void_mix(r, rng, share=0.05)
    want = pkg.rays_host(now, sp, r, radius, with_info=True, **kw)
    RS.same_hits(f.raycast(r, radius, **kw), want, str(what))
    info = f.rays_info()
    assert (info.rays, info.hits, info.voidRays, info.flags) == (m, want[4].hits, want[4].voidRays, want[4].flags)
    # the host's copy of the walk, and the other flags on the same state
    RS.same_hits(pkg.rays_host(now, sp, r, radius, walk=True, **kw), want, str(what) + " (walk on the host)")
    other = dict(fluid_only=not kw["fluid_only"], any_hit=False)
    f.set_option(pkg.SPH_OPT_RAYS_VARIANT, 1 - variant)
    RS.same_hits(f.raycast(r, radius, **other), pkg.rays_host(now, sp, r, radius, **other), str(what) + f" {other}")
    f.close()
