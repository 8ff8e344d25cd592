"""Ray casts on the CPU: sph_rays_host (the definition: brute force over all participating records with the engine's ray_hit) against
the float64 statement of rays_ref.py, exact cases by hand, windows, void rays, participation, flags, layouts and refusals.

Measured here for the t of the twin on the four uniform scenes below (4096 segments each): the largest |t32 - t64| / max(|t64|, 1e-3)
is 1.07e-5 (r = 0.25, 1200 records); the test asserts 4 x that, 4.3e-5 (rounding headroom: the scenes are fixed).  rays_ref named
0.1 %, 0.02 %, 0 % and 0.02 % of the rays, with no disagreement in id or hit / miss outside them."""
import ctypes as C

import numpy as np
import pytest

import rays_ref as RR
import rays_scenes as RS
from support import records

F = np.float32
INF = np.inf
T_BOUND = 4.3e-5


@pytest.mark.parametrize("n,seed", [(300, 41), (1200, 42)])
@pytest.mark.parametrize("radius", [0.25, 0.1])
def test_twin_against_float64(pkg, n, seed, radius):
    rec, sp = RS.uniform(pkg, n, seed)
    r = RS.segments(np.random.default_rng(100 + n), sp, 4096)
    t, ids, pos, nrm, info = pkg.rays_host(rec, sp, r, radius, with_info=True)
    t64, id64, named = RR.cast(rec["pos"], r, radius)
    print("named", named.mean(), "hits", info.hits)
    assert named.mean() <= 0.01
    ok = ~named
    assert np.array_equal(ids[ok], id64[ok])
    hit = ok & (id64 >= 0)
    rel = np.abs(t[hit].astype(np.float64) - t64[hit]) / np.maximum(np.abs(t64[hit]), 1e-3)
    print("largest relative error of t", rel.max())
    assert rel.max() <= T_BOUND
    assert np.isposinf(t[ids < 0]).all() and (pos[ids < 0] == 0).all() and (nrm[ids < 0] == 0).all()
    assert info.rays == 4096 and info.hits == (ids >= 0).sum() and info.voidRays == 0 and info.flags == 0 and info.radius == F(radius)
    # pos = fmaf(t, d, o) lies on the sphere of its record; the normal is a unit vector
    h = ids >= 0
    x = rec["pos"][ids[h], :3].astype(np.float64)
    assert np.abs(np.linalg.norm(pos[h].astype(np.float64) - x, axis=1) - radius).max() < 1e-4
    assert np.abs(np.linalg.norm(nrm[h].astype(np.float64), axis=1) - 1.0).max() < 1e-3
    any_ = pkg.rays_host(rec, sp, r, radius, any_hit=True)
    assert np.array_equal(any_[1] == 0, ids >= 0) and np.array_equal(any_[1] == -1, ids < 0)
    assert (any_[0][h] == 0).all() and np.isposinf(any_[0][~h]).all() and (any_[2] == 0).all() and (any_[3] == 0).all()


def _row(rec, y, z):
    """ids of the lattice row along x at (y, z), ascending in x."""
    p = rec["pos"]
    i = np.flatnonzero((p[:, 1] == F(y)) & (p[:, 2] == F(z)))
    return i[np.argsort(p[i, 0])]


def test_exact_cases_on_the_lattice(pkg):
    rec, sp = RS.lattice(pkg)
    row = _row(rec, -0.5, 0.0)
    assert len(row) == 7 and rec["pos"][row[0], 0] == F(-0.5)
    # an axis ray through a row of spheres: the first one, t = distance - r exactly
    t, ids, pos, nrm = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.5, 0.0], [1, 0, 0]), 0.125)
    assert ids[0] == row[0] and t[0] == F(2.375) and pos[0].tolist() == [-0.625, -0.5, 0.0] and nrm[0].tolist() == [-1.0, 0.0, 0.0]
    # ... in units of the direction: nothing is normalised
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.5, 0.0], [4, 0, 0]), 0.125)
    assert ids[0] == row[0] and t[0] == F(2.375 / 4)
    # from the other side, a negative window: t may be negative when tmin is
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([3.0, -0.5, 0.0], [1, 0, 0], -10.0, 0.0), 0.125)
    assert ids[0] == row[0] and t[0] == F(-3.625)
    # midway between two rows at r = 0.25: both first spheres are entered at the same t, the smaller id wins
    other = _row(rec, -0.25, 0.0)
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.375, 0.0], [1, 0, 0]), 0.25)
    assert ids[0] == min(row[0], other[0])
    # windows: a tmin past the first sphere's entry gives the next sphere entered; a start inside a sphere skips it
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.5, 0.0], [1, 0, 0], 2.4), 0.125)
    assert ids[0] == row[1] and t[0] == F(2.625)
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-0.5, -0.5, 0.0], [1, 0, 0]), 0.125)          # starts at the centre of row[0]
    assert ids[0] == row[1] and t[0] == F(0.125)
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.5, 0.0], [1, 0, 0], 0.0, 2.25), 0.125)
    assert ids[0] == -1 and np.isposinf(t[0])
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([-3.0, -0.5, 0.0], [1, 0, 0], 0.0, 2.375), 0.125)  # tmax = t: accepted
    assert ids[0] == row[0]


def test_coincident_eight(pkg):
    rec, sp, same = RS.coincident(pkg)
    x = rec["pos"][same[0], :3]
    d = np.array([0.3, -0.2, 0.9], F)
    r = RS.rays(x - F(0.2) * d, d)                                                  # starts 0.19 away, outside r = 0.1
    t, ids, _, _ = pkg.rays_host(rec, sp, r, 0.1)
    t64, id64, _ = RR.cast(rec["pos"], r, 0.1)
    assert ids[0] == same[0] == id64[0]


VOID = [[np.nan, 0, 0, 0, 1, 0, 0, 1], [0, np.inf, 0, 0, 1, 0, 0, 1], [0, 0, 0, np.nan, 1, 0, 0, 1], [0, 0, 0, -np.inf, 1, 0, 0, 1],
        [0, 0, 0, 0, np.nan, 0, 0, 1], [0, 0, 0, 0, 1, -np.inf, 0, 1], [0, 0, 0, 0, 1, 0, 0, np.nan], [0, 0, 0, 0, 0, 0, 0, 1],
        [0, 0, 0, 0, 1e-30, 0, 0, 1], [0, 0, 0, 0, 3e38, 3e38, 0, 1], [0, 0, 0, 2, 1, 0, 0, 1]]


def test_void_rays(pkg):
    """Each kind: non-finite o, d, tmin; NaN tmax; a zero (also by underflow) or not finite; tmin > tmax."""
    rec, sp = RS.uniform(pkg, 300, 41)
    r = np.array(VOID, F)
    r[:, 0:3] += rec["pos"][5, :3] - np.array([0.5, 0, 0], F)                       # the finite ones would hit record 5 or its neighbours
    assert RR.void(r).all()
    t, ids, pos, nrm, info = pkg.rays_host(rec, sp, r, 0.25, with_info=True)
    assert (ids == -1).all() and np.isposinf(t).all() and (pos == 0).all() and info.voidRays == len(r) and info.hits == 0
    good = RS.rays(rec["pos"][5, :3] - np.array([0.5, 0, 0], F), [1, 0, 0], 0.0, INF)
    _, ids, _, _, info = pkg.rays_host(rec, sp, good, 0.25, with_info=True)
    assert ids[0] >= 0 and info.voidRays == 0


def test_records_outside_the_grid_neither_hit_nor_block(pkg):
    sp = RS.params(pkg)
    lo, dims, cs = RS.grid(pkg, sp)
    hi = lo + dims.astype(F) * cs
    inside = np.array([0.25, -0.5, 0.125], F)
    pos = np.array([inside, [hi[0] + F(0.3), -0.5, 0.125], [lo[0] - F(0.01), -0.5, 0.125], [np.nan, -0.5, 0.125]], F)
    rec = records(pkg, pos, np.zeros_like(pos))
    r = np.concatenate([RS.rays([hi[0] + 2, -0.5, 0.125], [-1, 0, 0]), RS.rays([lo[0] - 2, -0.5, 0.125], [1, 0, 0])])
    t, ids, _, _ = pkg.rays_host(rec, sp, r, 0.25)
    assert ids.tolist() == [0, 0]                                                   # records 1 and 2 stand in front and are passed through
    t, ids, _, _ = pkg.rays_host(rec[1:], sp, r, 0.25)
    assert ids.tolist() == [-1, -1]
    # inside the last cell: takes part (the test is k_bin's fp32 quotient, so "inside" is decided after its rounding)
    pos[1, 0] = hi[0] - F(0.001)
    t, ids, _, _ = pkg.rays_host(records(pkg, pos, np.zeros_like(pos)), sp, r, 0.25)
    assert ids[0] == 1


def test_fluid_only(pkg):
    rec, sp = RS.with_ghosts(pkg)
    r = RS.segments(np.random.default_rng(5), sp, 2048)
    ghost = rec["isGhost"] != 0
    t, ids, _, _ = pkg.rays_host(rec, sp, r, 0.25)
    tf, idf, _, _, info = pkg.rays_host(rec, sp, r, 0.25, fluid_only=True, with_info=True)
    assert ghost[ids[ids >= 0]].any() and not ghost[idf[idf >= 0]].any() and info.flags == pkg.SPH_RAYS_FLUID_ONLY
    assert (rec["isActive"][ids[ids >= 0]] == 0).any()                             # inactive records take part like any other
    # the same as casting against the fluid records alone
    keep = np.flatnonzero(~ghost)
    tk, idk, _, _ = pkg.rays_host(rec[keep], sp, r, 0.25)
    assert np.array_equal(np.where(idk >= 0, keep[np.maximum(idk, 0)], -1), idf) and tk.tobytes() == tf.tobytes()
    t64, id64, named = RR.cast(rec["pos"], r, 0.25, takes_part=~ghost)
    assert np.array_equal(idf[~named], id64[~named])


def test_layouts(pkg):
    assert C.sizeof(pkg.SphRayHit) == 32 and C.sizeof(pkg.SphRaysInfo) == 32 and pkg.RAY_HIT_DTYPE.itemsize == 32
    assert [pkg.RAY_HIT_DTYPE.fields[k][1] for k in ("t", "id", "pos", "normal")] == [0, 4, 8, 20]
    assert (pkg.SphRaysInfo.rays.offset, pkg.SphRaysInfo.hits.offset, pkg.SphRaysInfo.voidRays.offset, pkg.SphRaysInfo.radius.offset,
            pkg.SphRaysInfo.flags.offset) == (0, 8, 16, 24, 28)
    assert (pkg.SPH_RAYS_FLUID_ONLY, pkg.SPH_RAYS_ANY_HIT) == (1, 2)


def test_refusals_and_empty_calls(pkg):
    L = pkg.load_library()
    rec, sp = RS.uniform(pkg, 300, 41)
    cs = float(RS.grid(pkg, sp)[2])
    r = RS.segments(np.random.default_rng(1), sp, 4)
    info = pkg.SphRaysInfo()
    vp = C.c_void_p
    hits = np.zeros(4, pkg.RAY_HIT_DTYPE)
    call = lambda radius, flags=0, m=4, rp=r.ctypes.data_as(vp), pp=rec.ctypes.data_as(vp), out=C.byref(info): \
        L.sph_rays_host(pp, len(rec), C.byref(sp), rp, m, radius, flags, hits.ctypes.data_as(vp), out)
    assert call(0.25) == 0 and info.rays == 4
    assert call(0.5 * cs) == 0                                                      # half a cell exactly is allowed
    for bad in (0.0, -0.1, float("nan"), float("inf"), float(np.nextafter(F(0.5 * cs), F(1)))):
        assert call(bad) == -1, bad
    assert call(0.25, flags=4) == -1 and call(0.25, m=1 << 31) == -1
    assert call(0.25, rp=None) == -1 and call(0.25, pp=None) == -1 and call(0.25, out=None) == -1
    assert L.sph_rays_host(rec.ctypes.data_as(vp), len(rec), None, r.ctypes.data_as(vp), 4, 0.25, 0, None, C.byref(info)) == -1
    assert L.sph_rays_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), r.ctypes.data_as(vp), 4, 0.25, 0, None, C.byref(info)) == 0   # hits may be null
    with pytest.raises(pkg.SphError):
        pkg.rays_host(rec, sp, np.zeros((3, 7), F), 0.25)
    # m = 0 and n = 0
    t, ids, pos, nrm, info = pkg.rays_host(rec, sp, np.zeros((0, 8), F), 0.25, with_info=True)
    assert t.shape == (0,) and pos.shape == (0, 3) and info.rays == 0 and info.hits == 0
    t, ids, _, _, info = pkg.rays_host(rec[:0], sp, r, 0.25, with_info=True)
    assert (ids == -1).all() and np.isposinf(t).all() and info.rays == 4 and info.hits == 0


def test_ray_builders(pkg):
    cam = pkg.camera_rays((0, 0, 5), (0, 0, 0), (0, 1, 0), np.pi / 2, 5, 3)
    assert cam.shape == (15, 8) and cam.dtype == F and (cam[:, 0:3] == [0, 0, 5]).all() and (cam[:, 3] == 0).all() and np.isposinf(cam[:, 7]).all()
    assert np.allclose(cam[7, 4:7], [0, 0, -1], atol=1e-7)                           # the centre pixel looks along the axis
    assert np.allclose(cam[0, 4:7], [-(4 / 5) * (5 / 3), 2 / 3, -1], atol=1e-6)      # top left: x to the left, y up
    assert np.allclose(cam[14, 4:7], [(4 / 5) * (5 / 3), -2 / 3, -1], atol=1e-6)
    sheet = pkg.parallel_rays((0, 4, 0), (2, 0, 0), (0, 0, 3), (0, -1, 0), 4, 3, tmax=9.0)
    assert sheet.shape == (12, 8) and (sheet[:, 4:7] == [0, -1, 0]).all() and (sheet[:, 7] == 9).all()
    assert sheet[0, 0:3].tolist() == [0.25, 4.0, 0.5] and sheet[5, 0:3].tolist() == [0.75, 4.0, 1.5] and sheet[11, 0:3].tolist() == [1.75, 4.0, 2.5]
    # a sheet straight down onto the lattice: the centre ray meets the top of a column
    rec, sp = RS.lattice(pkg)
    col = np.flatnonzero((rec["pos"][:, 0] == F(0.25)) & (rec["pos"][:, 2] == F(0.0)))
    top = col[np.argmax(rec["pos"][col, 1])]
    down = pkg.parallel_rays((0.25 - 0.5, 3.0, -0.5), (1, 0, 0), (0, 0, 1), (0, -1, 0), 1, 1)
    t, ids, pos, nrm = pkg.rays_host(rec, sp, down, 0.125)
    assert ids[0] == top and nrm[0].tolist() == [0.0, 1.0, 0.0] and t[0] == F(3.0 - 0.25 - 0.125)


def test_the_walk_on_the_host_equals_the_definition(pkg):
    """sph_rays_walk_host runs the device's ray_walk over a grid built on the host: on every scene the GPU tests use it gives the
    bytes of the brute force."""
    total = hits = 0
    for name, rec, sp, casts in RS.scenes(pkg):
        for r, radius, kw in casts:
            want = pkg.rays_host(rec, sp, r, radius, with_info=True, **kw)
            got = pkg.rays_host(rec, sp, r, radius, with_info=True, walk=True, **kw)
            RS.same_hits(got, want, f"{name} r {radius} {kw}")
            assert (got[4].rays, got[4].hits, got[4].voidRays) == (want[4].rays, want[4].hits, want[4].voidRays)
            total += len(r)
            hits += int(want[4].hits)
        print(name, [(len(r), int((pkg.rays_host(rec, sp, r, radius, **kw)[1] >= 0).sum())) for r, radius, kw in casts])
    assert hits > total // 4
