"""Seeded random scenes (support.random_scene: kernel lengths, grids down to three cells, clumps, ghosts, particles outside the grid,
every container shape) after a few dispatches: the device's free-surface rows and ids are sph_shell_host's bytes on the downloaded
records, with radius, threshold, minCount and flags drawn from the seed."""
import numpy as np
import pytest

from support import random_scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_random_scene(pkg, seed):
    rec, sp, steps, what = random_scene(pkg, seed)
    rng = np.random.default_rng(9000 + seed)
    R = float(F(rng.choice([0.5, 1.0, 1.3, 2.0, 2.5, 3.0])) * F(sp.param_h))
    kw = dict(offset=float(rng.choice([0.0, 0.05, 0.10, 0.25])), min_count=int(rng.choice([0, 0, 8, 40])), fluid_only=bool(rng.integers(2)))
    print(what, "R", R, kw)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    for _ in range(2):
        f.DispatchN(steps)
    now = f.download()
    w_rows, w_ids, w_info = pkg.shell_host(now, sp, R, **kw)
    rows, ids = f.shell(R, **kw)
    info = f.shell_info()
    assert rows.tobytes() == w_rows.tobytes() and np.array_equal(ids, w_ids)
    assert (info.rows, info.numShell, info.numIsolated, info.maxCount, info.stencil, info.flags, info.kind) == \
        (w_info.rows, w_info.numShell, w_info.numIsolated, w_info.maxCount, w_info.stencil, w_info.flags, 1)
    # a query list on the same state
    pts = now["pos"][:: max(1, len(now) // 257), :3] + F(0.1) * F(sp.param_h)
    q = f.query_shell(pts, R, **kw)
    w = pkg.shell_host(now, sp, R, points=pts, **kw)
    assert q[0].tobytes() == w[0].tobytes() and np.array_equal(q[1], w[1])
    f.close()
