"""Scenes and rays shared by the ray-cast tests (test_rays_cpu.py, test_gpu_rays.py, test_gpu_fuzz_rays.py): the box of 4 x 3 x 3.5
at h = 0.5 of query_scenes.py with its uniform clouds, exact lattice, coincident eight and ghost mix, plus a lattice that fills the
whole grid and the families of rays that can go wrong in a grid walk."""
from importlib import import_module

import numpy as np

from conftest import PKG_NAME
from query_scenes import box_cloud, coincident, grid, grid_cloud, lattice, params, uniform, with_ghosts  # noqa: F401
from support import records

F = np.float32
INF = np.inf
# the feature's symbols, at import: on a tree without ray casts every test file that imports this module fails here
_pkg = import_module(PKG_NAME)
SPH_RAYS_FLUID_ONLY, SPH_RAYS_ANY_HIT, RAY_HIT_DTYPE = _pkg.SPH_RAYS_FLUID_ONLY, _pkg.SPH_RAYS_ANY_HIT, _pkg.RAY_HIT_DTYPE


def rays(o, d, tmin=0.0, tmax=INF):
    """(m, 8) float32 rays from (m, 3) origins and directions."""
    o, d = np.atleast_2d(np.asarray(o, F)), np.atleast_2d(np.asarray(d, F))
    m = max(len(o), len(d))
    r = np.zeros((m, 8), F)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def segments(rng, sp, m, tmax=1.0):
    """m segments from uniform points of the container box scaled by two toward uniform points inside it: d = target - origin, so that
    t = 1 is the target."""
    c = np.array(list(sp.param_boxCenter), F)
    half = np.array(list(sp.param_boxHalf), F)
    o = c + (rng.random((m, 3)).astype(F) * F(2.0) - F(1.0)) * F(2.0) * half
    target = box_cloud(rng, sp, m)
    return rays(o, target - o, 0.0, tmax)


def dense_lattice(pkg, seed=14):
    """Particles on every multiple of h / 2 strictly inside the grid's box, ids shuffled: with r = h / 2 the spheres overlap, every ray
    meets many, and a walk that stops too early returns a later one."""
    sp = params(pkg)
    lo, dims, cs = grid(pkg, sp)
    ax = [lo[a] + F(0.25) * np.arange(1, 2 * int(dims[a]), dtype=F) for a in range(3)]
    pos = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    pos = pos[np.random.default_rng(seed).permutation(len(pos))]
    return records(pkg, pos, np.zeros_like(pos)), sp


DIRECTIONS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1],                # two zero components
                       [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, -1, 0], [0, -1, 1], [-1, 0, -1], [2, 1, 0], [0, 1, -3],   # one zero component
                       [1, 1, 1], [-1, 1, 1], [1, -1, -1], [-1, -1, -1], [1, 2, 3]], F)


def lattice_rays(sp_grid, rng, per=12):
    """Rays along cell faces, along cell edges and through cell corners: through `per` random cell corners of the grid, every direction
    of DIRECTIONS, starting outside the grid's box (8 directions back) with tmax = +inf; the same through face centres (one coordinate
    on a face) and through edge midpoints (two on faces)."""
    lo, dims, cs = sp_grid
    out = []
    for kind in range(3):                                                         # 0: corners, 1: edge midpoints, 2: face centres
        idx = np.stack([rng.integers(0, int(dims[a]) + 1, per) for a in range(3)], axis=1).astype(F)
        off = np.zeros((per, 3), F)
        for j in range(per):
            axes = rng.permutation(3)[:kind]
            off[j, axes] = F(0.5)
        through = lo + (idx + off) * cs
        for d in DIRECTIONS:
            out.append(rays(through - F(8.0) * d, np.broadcast_to(d, through.shape), 0.0, INF))
    return np.concatenate(out)


def face_huggers(pkg, seed=15, per=40):
    """Particles within 0.05 of every face of the grid's box (inside it), and rays that run OUTSIDE the box, 0.1 beyond each face and
    parallel to it: they can only meet the part of a sphere of r = 0.25 that sticks out."""
    sp = params(pkg)
    lo, dims, cs = grid(pkg, sp)
    hi = lo + dims.astype(F) * cs
    rng = np.random.default_rng(seed)
    pos, out = [], []
    for a in range(3):
        for side in (0, 1):
            p = grid_cloud(rng, (lo, dims, cs), per)
            p[:, a] = lo[a] + F(0.05) * rng.random(per).astype(F) if side == 0 else hi[a] - F(0.001) - F(0.05) * rng.random(per).astype(F)
            pos.append(p)
            b = (a + 1) % 3
            o = p.copy()
            o[:, a] = lo[a] - F(0.1) if side == 0 else hi[a] + F(0.1)
            o[:, b] = lo[b] - F(1.0)
            d = np.zeros((per, 3), F)
            d[:, b] = 1
            out.append(rays(o, d))
            d2 = d.copy()
            d2[:, (a + 2) % 3] = F(0.01)                                         # nearly parallel, one zero component
            out.append(rays(o, d2))
    pos = np.concatenate(pos)
    return records(pkg, pos, np.zeros_like(pos)), sp, np.concatenate(out)


def plane_scene(pkg, seed=16, n=800, m=600):
    """Particles whose y lies exactly on cell planes (so they belong to the cell ABOVE the plane), x and z uniform; rays in the xz
    plane at 0.2499 below or above a plane: with r = 0.5f * cellSize exactly the ray's own cell is the neighbour of the neighbour of the
    centre's cell on one side and the centre's own on the other."""
    sp = params(pkg)
    lo, dims, cs = grid(pkg, sp)
    rng = np.random.default_rng(seed)
    pos = grid_cloud(rng, (lo, dims, cs), n)
    pos[:, 1] = lo[1] + rng.integers(1, int(dims[1]), n).astype(F) * cs
    o = grid_cloud(rng, (lo, dims, cs), m)
    o[:, 1] = lo[1] + rng.integers(1, int(dims[1]), m).astype(F) * cs + np.where(rng.random(m) < 0.5, F(-0.2499), F(0.2499))
    d = rng.standard_normal((m, 3)).astype(F)
    d[:, 1] = 0
    d[: m // 3, 0] = 0                                                             # a third along z only
    d[m // 3: 2 * m // 3, 2] = 0                                                   # a third along x only
    return records(pkg, pos, np.zeros_like(pos)), sp, rays(o - F(6.0) * d / np.linalg.norm(d, axis=1, keepdims=True).astype(F), d)


def void_mix(r, rng, share=0.1):
    """A copy of rays r in which about `share` of them are void, one kind each."""
    r = r.copy()
    kinds = [(0, np.nan), (1, np.inf), (3, np.nan), (3, -np.inf), (4, np.nan), (5, -np.inf), (7, np.nan), (None, 0.0), (3, 1e30)]
    for i in np.flatnonzero(rng.random(len(r)) < share):
        col, val = kinds[int(rng.integers(len(kinds)))]
        if col is None:
            r[i, 4:7] = 0
        elif col == 3 and val == 1e30:
            r[i, 3], r[i, 7] = 2.0, 1.0                                           # tmin > tmax
        else:
            r[i, col] = val
    return r


def scenes(pkg):
    """[(name, records, params, [(rays, radius, kwargs), ...])]: everything the device (and the host's copy of its walk) is compared
    with the definition on.  Radii are exact in fp32; 0.25 is 0.5f * cellSize exactly."""
    rng = np.random.default_rng(77)
    out = []
    rec, sp = uniform(pkg, 1200, 42)
    g = grid(pkg, sp)
    seg = segments(np.random.default_rng(1300), sp, 4096)
    inside = rays(box_cloud(rng, sp, 1024), rng.standard_normal((1024, 3)).astype(F), 0.0, INF)       # start inside, leave the box, tmax = +inf
    far = segments(rng, sp, 1024, tmax=INF)
    far[:, 0:3] = far[:, 0:3] * F(6.0)                                              # start well outside the grid's box
    far[:, 4:7] = box_cloud(rng, sp, 1024) - far[:, 0:3]
    win = segments(rng, sp, 1024)
    win[:, 3], win[:, 7] = F(0.3) + F(0.4) * rng.random(1024).astype(F), F(0.6) + F(0.6) * rng.random(1024).astype(F)
    neg = inside.copy()
    neg[:, 3], neg[:, 7] = F(-50.0), F(0.5)
    lat = lattice_rays(g, rng)
    out.append(("uniform 1200", rec, sp, [(seg, 0.25, {}), (seg, 0.1, {}), (inside, 0.25, {}), (far, 0.25, {}), (win, 0.1, {}), (neg, 0.25, {}),
                                          (lat, 0.25, {}), (void_mix(seg, rng), 0.25, {}), (seg, 0.25, dict(any_hit=True)),
                                          (void_mix(inside, rng), 0.1, dict(any_hit=True)), (seg[:0], 0.25, {})]))
    rec, sp = lattice(pkg)
    out.append(("lattice", rec, sp, [(lat, 0.125, {}), (lat, 0.25, {}), (seg[:1024], 0.125, {}), (lat, 0.25, dict(any_hit=True))]))
    rec, sp, fr = face_huggers(pkg)
    out.append(("face huggers", rec, sp, [(fr, 0.25, {}), (lat, 0.25, {}), (fr, 0.1, {})]))
    pos = grid_cloud(rng, g, 1500, beyond=0.2)
    out.append(("clamped records", records(pkg, pos, np.zeros_like(pos)), sp, [(seg, 0.25, {}), (far, 0.1, {}), (lat, 0.25, {}), (inside, 0.25, {})]))
    rec, sp, pr = plane_scene(pkg)
    out.append(("planes, r = half a cell", rec, sp, [(pr, 0.25, {}), (lat, 0.25, {})]))
    rec, sp = dense_lattice(pkg)
    out.append(("dense lattice", rec, sp, [(seg[:2048], 0.25, {}), (lat, 0.25, {}), (inside, 0.125, {}), (far, 0.25, {})]))
    rec, sp, same = coincident(pkg)
    x = rec["pos"][same[0], :3]
    d = rng.standard_normal((256, 3)).astype(F)
    out.append(("coincident", rec, sp, [(rays(x - F(2.0) * d, d), 0.1, {}), (seg[:1024], 0.25, {})]))
    rec, sp = with_ghosts(pkg)
    out.append(("ghosts", rec, sp, [(seg, 0.25, {}), (seg, 0.25, dict(fluid_only=True)), (seg, 0.1, dict(fluid_only=True, any_hit=True))]))
    return out


def same_hits(got, want, what):
    """(t, ids, pos, normal) byte for byte."""
    for a, b, name in zip(got[:4], want[:4], ("t", "ids", "pos", "normal")):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint32).reshape(len(a), -1) != b.view(np.uint32).reshape(len(b), -1)).any(axis=1))
            raise AssertionError(f"{what}: {name} differs on {len(bad)} of {len(a)} rays, first {bad[:5].tolist()}: {a[bad[:3]].tolist()} against {b[bad[:3]].tolist()}")
