"""Seeded random scenes (support.random_scene: kernel lengths, grids down to three cells, clumps, ghosts, particles outside the grid,
every container shape) after a few dispatches: the device's k nearest neighbours are sph_knn_host's bytes on the downloaded records,
with k, radius, flags and the kernel variant drawn from the seed."""
import numpy as np
import pytest

from support import random_scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_random_scene(pkg, seed):
    rec, sp, steps, what = random_scene(pkg, seed)
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.choice([1, 3, 8, 9, 16, 17, 24, 32, 33, 50, 64]))
    R = float(F(rng.choice([0.5, 1.0, 1.5, 2.0, 2.5, 3.0])) * F(sp.param_h))
    kw = dict(self_=bool(rng.integers(2)), fluid_only=bool(rng.integers(2)))
    variant = int(rng.integers(2))
    print(what, "k", k, "R", R, kw, "variant", variant)
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_KNN_VARIANT, variant)
    for _ in range(2):
        f.DispatchN(steps)
    now = f.download()
    w_idx, w_d2, w_cnt, w_info = pkg.knn_host(now, sp, k, R, **kw)
    idx, d2, cnt = f.knn(k, R, **kw)
    info = f.knn_info()
    assert cnt.tobytes() == w_cnt.tobytes() and idx.tobytes() == w_idx.tobytes() and d2.view(np.uint32).tobytes() == w_d2.view(np.uint32).tobytes()
    assert (info.rows, info.total, info.rowsFull, info.k, info.stencil, info.flags, info.kind) == \
        (w_info.rows, w_info.total, w_info.rowsFull, k, w_info.stencil, w_info.flags, 1)
    # the other variant and a query list on the same state
    f.set_option(pkg.SPH_OPT_KNN_VARIANT, 1 - variant)
    assert f.knn(k, R, **kw)[0].tobytes() == w_idx.tobytes()
    pts = now["pos"][:: max(1, len(now) // 257), :3] + F(0.1) * F(sp.param_h)
    q = f.query_knn(pts, k, R, fluid_only=kw["fluid_only"])
    w = pkg.knn_host(now, sp, k, R, points=pts, fluid_only=kw["fluid_only"])
    assert q[2].tobytes() == w[2].tobytes() and q[0].tobytes() == w[0].tobytes() and q[1].view(np.uint32).tobytes() == w[1].view(np.uint32).tobytes()
    f.close()
