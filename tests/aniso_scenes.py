"""Scenes shared by the tests of the anisotropic kernels (test_aniso_cpu.py, test_gpu_aniso.py) beside those of shell_scenes.py and
query_scenes.py: the degenerate neighbourhoods (one jittered layer, a line, a few particles) at h = 0.28 with spacing dx = h / 2.4, and
the lattices the field is compared on."""
import numpy as np

import shell_scenes as SS
from support import records

F = np.float32
H, DX = SS.H, SS.DX


def layer(pkg, side=24, seed=7):
    """side x side particles in the plane z = 0, jittered by +-0.2 dx along every axis: (records, params, nominal in dx)."""
    ax = np.arange(side, dtype=np.float64) - (side - 1) / 2.0
    g = np.stack(np.meshgrid(ax, ax, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    return SS._scene(pkg, g, seed)


def line(pkg, count=40, seed=8):
    """count particles along x, jittered by +-0.2 dx along every axis."""
    g = np.zeros((count, 3))
    g[:, 0] = np.arange(count) - (count - 1) / 2.0
    return SS._scene(pkg, g, seed)


def few(pkg, count):
    """count particles half a dx apart along the diagonal, no jitter."""
    pos = (np.arange(count, dtype=np.float64)[:, None] * np.array([0.5, 0.25, -0.25]) * DX).astype(F)
    return records(pkg, pos, np.zeros_like(pos)), SS.params(pkg)


def ball_lattice(pkg, sp, overhang=False):
    """(origin, spacing, dims) of spacing h / 2 around the ball of 5 spacings: a box of +-7 dx, or with `overhang` a bar of 7 x 7 nodes
    through the ball's centre that starts two cells outside the grid's lower x face (its first nodes fall into clamped cells)."""
    s = float(F(sp.param_h) / F(2))
    if not overhang:
        lo = -7.0 * DX
        n = int(np.ceil(14.0 * DX / s)) + 1
        return (lo, lo, lo), (s, s, s), (n, n, n)
    g = pkg.compute_grid_extents(sp)
    x0 = float(g.gridMin[0]) - 2.0 * float(g.cellSize)
    return (x0, -3.0 * s, -3.0 * s), (s, s, s), (int(np.ceil((7.0 * DX - x0) / s)) + 1, 7, 7)


def face_lattice():
    """The columns of the flatness statement on the block's +z face: 17 x 17 columns within +-4 dx of the axis, nodes every dx / 8 from
    7 dx to 12 dx.  (origin, spacing, dims, zs in dx)."""
    origin = (-4.0 * DX, -4.0 * DX, 7.0 * DX)
    spacing = (0.5 * DX, 0.5 * DX, DX / 8.0)
    dims = (17, 17, 41)
    zs = (F(origin[2]) + np.arange(dims[2], dtype=F) * F(spacing[2])).astype(np.float64) / DX
    return origin, spacing, dims, zs
