"""Scenes shared by the tests of the spatial queries (neighbour lists, components, k nearest neighbours, ray casts, free-surface shell,
on the CPU and on the device): a box of 4 x 3 x 3.5 at h = 0.5, uniform clouds, the exact lattice, coincident particles, ghosts of every
kind, the crowded cell and the query cloud with its three non-finite rows."""
import numpy as np

import neighbors_ref as NR
from support import records

F = np.float32


def params(pkg, h=0.5, half=(2.0, 1.5, 1.75), cap=160):
    return pkg.default_params(param_h=h, param_boxHalf=half, param_boxCenter=(0.25, -0.5, 0.125), grid_cap=cap)


def grid(pkg, sp):
    g = pkg.compute_grid_extents(sp)
    return np.array(list(g.gridMin), F), np.array(list(g.dims), np.int64), F(g.cellSize)


def box_cloud(rng, sp, n):
    """n uniform positions inside the container box (4 x 3 x 3.5 by default)."""
    c = np.array(list(sp.param_boxCenter), F)
    half = np.array(list(sp.param_boxHalf), F)
    return c + (rng.random((n, 3)).astype(F) * F(2.0) - F(1.0)) * half


def grid_cloud(rng, sp_grid, n, beyond=0.0):
    """n uniform positions over the grid's box, widened by `beyond` of its extent on every side (clamped cells)."""
    lo, dims, cs = sp_grid
    ext = dims.astype(F) * cs
    return lo + (rng.random((n, 3)).astype(F) * F(1.0 + 2.0 * beyond) - F(beyond)) * ext


def uniform(pkg, n, seed):
    sp = params(pkg)
    pos = box_cloud(np.random.default_rng(seed), sp, n)
    return records(pkg, pos, np.zeros_like(pos)), sp


def lattice(pkg, seed=11, side=7):
    """side^3 particles on a lattice of spacing h / 2 with exactly representable coordinates (multiples of 1/4), ids shuffled: every
    difference and every r2 is exact in fp32 and in float64, so whole shells of candidates tie exactly and only the id orders them."""
    sp = params(pkg)
    ax = (np.arange(side, dtype=F) - F(side // 2)) * F(0.25)
    pos = np.stack(np.meshgrid(ax + F(0.25), ax + F(-0.5), ax + F(0.0), indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    return records(pkg, pos, np.zeros_like(pos)), sp


def coincident(pkg, seed=12, n=300, where=(0.3, -0.45, 0.2)):
    """Eight particles at one position (ids spread through the array) among a uniform background."""
    sp = params(pkg)
    rng = np.random.default_rng(seed)
    pos = box_cloud(rng, sp, n)
    same = np.sort(rng.choice(n, size=8, replace=False))
    pos[same] = np.array(where, F)
    return records(pkg, pos, np.zeros_like(pos)), sp, same


def with_ghosts(pkg, n=1200, seed=13):
    """A uniform cloud in which every third record is a ghost of kind 1 or 3 and every fourth record is inactive."""
    rec, sp = uniform(pkg, n, seed)
    i = np.arange(n)
    rec["isGhost"] = np.where(i % 3 == 0, np.where(i % 2 == 0, 1, 3), 0)
    rec["isActive"] = (i % 4 != 0)
    return rec, sp


def crowded_cell(pkg, crowd):
    """`crowd` particles inside cell (3, 2, 4) behind 400 uniform ones: (records, params, start, members), the cell's run of sorted
    slots (its first slot and its length, the background's share included).  The generator is seeded with `crowd`."""
    rng = np.random.default_rng(crowd)
    sp = params(pkg)
    lo, dims, cs = grid(pkg, sp)
    cell = np.array([3, 2, 4])
    assert (cell + 1 < dims).all()
    inside = lo + (cell.astype(F) + F(0.05) + F(0.9) * rng.random((crowd, 3)).astype(F)) * cs
    pos = np.concatenate([grid_cloud(rng, (lo, dims, cs), 400), inside])
    rec = records(pkg, pos, np.zeros_like(pos))
    c = NR.cells(pkg, rec["pos"], sp)
    mine = (cell[2] * dims[1] + cell[1]) * dims[0] + cell[0]
    start, members = int((c < mine).sum()), int((c == mine).sum())
    return rec, sp, start, members


def query_cloud(pkg, m=701):
    """1500 particles up to a tenth of the grid's extent beyond its faces and m query points up to 0.3 of it beyond them (701 is no
    multiple of 64), with NaN, +inf and -inf in rows 5, 256 and m - 1: (records, params, points)."""
    rng = np.random.default_rng(8)
    sp = params(pkg)
    g = grid(pkg, sp)
    pos = grid_cloud(rng, g, 1500, beyond=0.1)
    rec = records(pkg, pos, np.zeros_like(pos))
    pts = grid_cloud(rng, g, m, beyond=0.3)
    pts[5, 0] = np.nan
    pts[256, 1] = np.inf
    pts[m - 1, 2] = -np.inf
    return rec, sp, pts
