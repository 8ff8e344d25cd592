"""Seeded random scenes (support.random_scene: kernel lengths, grids down to three cells, clumps, ghosts, particles outside the grid,
every container shape) after a few dispatches: the device's anisotropy rows, info and lattice are sph_aniso_host's and
sph_aniso_lattice_host's bytes on the downloaded records, with the config drawn from the seed."""
import numpy as np
import pytest

from support import random_scene

pytestmark = pytest.mark.gpu
F = np.float32
INFO_FIELDS = ("rows", "numSparse", "numClamped", "maxCount", "radius", "support", "stencil", "maxReach", "reachStencil", "kind", "flags")


@pytest.mark.parametrize("seed", range(6))
def test_random_scene(pkg, seed):
    rec, sp, steps, what = random_scene(pkg, seed)
    rng = np.random.default_rng(9100 + seed)
    h = F(sp.param_h)
    kw = dict(radius=float(F(rng.choice([1.0, 1.3, 2.0, 2.5, 3.0])) * h), support=float(F(rng.choice([0.5, 1.0, 1.25])) * h),
              smoothing=float(rng.choice([0.0, 0.5, 0.9, 1.0])), max_ratio=float(rng.choice([1.0, 2.0, 4.0, 8.0])),
              max_stretch=float(rng.choice([1.0, 1.5])), min_count=int(rng.choice([0, 8, 25, 60])), sparse_scale=float(rng.choice([0.5, 1.0])),
              fluid_only=bool(rng.integers(2)))
    print(what, kw)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for _ in range(2):
        f.DispatchN(steps)
    now = f.download()
    w_rows, w_info = pkg.aniso_host(now, sp, **kw)
    rows = f.anisotropy(**kw)
    info = f.aniso_info()
    assert rows.tobytes() == w_rows.tobytes()
    assert [getattr(info, a) for a in INFO_FIELDS] == [getattr(w_info, a) for a in INFO_FIELDS]
    # a lattice over the grid's box and a quarter of a cell beyond it, on the same state (support <= 1.25 h keeps the reach inside three cells)
    g = pkg.compute_grid_extents(sp)
    dims = tuple(min(int(d) * 2 + 2, 24) for d in g.dims)
    origin = tuple(float(F(x) - F(0.25) * F(g.cellSize)) for x in g.gridMin)
    spacing = float(F(g.cellSize) * F(0.5))
    if w_info.maxReach <= F(3) * F(g.cellSize):
        want, l_info = pkg.aniso_lattice_host(now, sp, origin, spacing, dims, **kw)
        got = f.aniso_lattice(origin, spacing, dims, **kw)
        assert got.tobytes() == want.tobytes()
        assert [getattr(f.aniso_info(), a) for a in INFO_FIELDS] == [getattr(l_info, a) for a in INFO_FIELDS]
    else:                                                                          # both sides refuse a reach above three cells
        for call in (lambda: pkg.aniso_lattice_host(now, sp, origin, spacing, dims, **kw), lambda: f.aniso_lattice(origin, spacing, dims, **kw)):
            with pytest.raises(pkg.SphError, match="maxReach"):
                call()
    f.close()
