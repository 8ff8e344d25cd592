"""Ray spans on the CPU: sph_rays_span_host (the definition: brute force over all participating records with the engine's ray_span)
against the numpy restatement of ray_spans_ref.py byte for byte, the two span walks (sph_rays_span_walk_host: the device's
ray_span_walk, layer and block, over a grid built on the host) against the definition byte for byte on every scene of rays_scenes.py,
and exact cases by hand: the lattice, windows, the coincident eight, clamped records, void rays and the info sums.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ray_spans_ref as SR
import rays_scenes as RS
from support import records, same_info as support_same_info

F = np.float32
INF = np.inf
FIELDS = ("tEnter", "tExit", "idEnter", "idExit", "count", "flags", "length")


same_rows, info_of_rows, _scenes = SR.same_rows, SR.info_of_rows, SR.scenes


def same_info(got, want, what):
    support_same_info(got, want, SR.INFO_FIELDS, what)


@pytest.mark.parametrize("which", range(8))
def test_walks_and_restatement_against_the_definition(pkg, which):
    """Every scene, every set of rays of it without any_hit (fluid_only kept): both walks give the definition's bytes, and the
    definition gives those of the numpy restatement.  A differing ray is a walk that missed or double-counted a sphere."""
    assert len(_scenes(pkg)) == 8                                                  # (the parametrisation covers every scene)
    name, rec, sp, casts = _scenes(pkg)[which]
    g = RS.grid(pkg, sp)
    crossed = 0
    for r, radius, kw in casts:
        what = f"{name} r {radius} {kw}"
        want, info = pkg.ray_spans_host(rec, sp, r, radius, with_info=True, **kw)
        info_of_rows(want, info, what)
        for variant in (0, 1):
            got, winfo = pkg.ray_spans_walk_host(rec, sp, r, radius, with_info=True, variant=variant, **kw)
            same_rows(got, want, f"{what} walk variant {variant}")
            same_info(winfo, info, f"{what} walk variant {variant}")
        ref = SR.spans(rec["pos"], r, radius, pkg.RAY_SPAN_DTYPE, takes_part=SR.takes_part(rec, g, kw.get("fluid_only", False)))
        same_rows(want, ref, f"{what} restatement")
        crossed += int(info.crossed)
    print(name, "crossed rays", crossed)
    assert crossed > 0


def _axis_row(rec, axis, through):
    """ids of the lattice row along `axis` through the point `through`, ascending along the axis."""
    p = rec["pos"][:, :3]
    others = [a for a in range(3) if a != axis]
    i = np.flatnonzero((p[:, others[0]] == F(through[others[0]])) & (p[:, others[1]] == F(through[others[1]])))
    return i[np.argsort(p[i, axis])]


@pytest.mark.parametrize("radius", [0.125, 0.25])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_lattice(pkg, axis, radius):
    """A ray along an axis through a row of seven centres: seven whole diameters, exact end points; cut at the fourth centre: three
    diameters and a half.  At r = 0.25 the rows beside it are touched in one point each (s == 0, thc == 0) and are not crossed."""
    rec, sp = RS.lattice(pkg)
    through = np.array([0.25, -0.5, 0.0], F)
    row = _axis_row(rec, axis, through)
    assert len(row) == 7
    x = rec["pos"][row, axis]
    o = through.copy()
    o[axis] = x[0] - F(3.0)
    d = np.zeros(3, F)
    d[axis] = 1
    for variant in (None, 0, 1):
        fn = (lambda r: pkg.ray_spans_host(rec, sp, r, radius)) if variant is None else (lambda r: pkg.ray_spans_walk_host(rec, sp, r, radius, variant=variant))
        s = fn(RS.rays(o, d))[0]
        assert s["count"] == 7 and s["length"] == 7 << 24 and s["flags"] == 0
        assert s["tEnter"] == F(3.0 - radius) and s["tExit"] == F(3.0 + 1.5 + radius) and s["idEnter"] == row[0] and s["idExit"] == row[6]
        s = fn(RS.rays(o, d, 0.0, float(x[3] - o[axis])))[0]                       # the window ends at the fourth centre
        assert s["count"] == 4 and s["length"] == 7 << 23 and s["tExit"] == F(3.75)
        assert s["idExit"] == (row[3] if radius == 0.125 else min(row[2], row[3]))  # (at r = 0.25 the third sphere ends at that centre too: the smaller id)
        s = fn(RS.rays(o, -d, -100.0, 0.0))[0]                                     # the same row in a negative window, direction reversed
        assert s["count"] == 7 and s["length"] == 7 << 24 and s["tEnter"] == F(-(4.5 + radius)) and s["tExit"] == F(-(3.0 - radius))
        assert s["idEnter"] == row[6] and s["idExit"] == row[0]
    assert pkg.ray_thickness(pkg.ray_spans_host(rec, sp, RS.rays(o, d), radius), radius)[0] == 7 * 2 * radius


def test_windows(pkg):
    rec, sp = RS.lattice(pkg)
    row = _axis_row(rec, 0, (0.25, -0.5, 0.0))
    x0 = float(rec["pos"][row[0], 0])                                              # -0.5
    span = lambda r, radius=0.125: pkg.ray_spans_host(rec, sp, r, radius)[0]
    # a start at a centre: the sphere counts, with tEnter == tmin and half a diameter; the cast ignores that sphere
    s = span(RS.rays([x0, -0.5, 0.0], [1, 0, 0]))
    assert s["count"] == 7 and s["tEnter"] == 0 and s["idEnter"] == row[0] and s["length"] == (13 << 23)
    t, ids, _, _ = pkg.rays_host(rec, sp, RS.rays([x0, -0.5, 0.0], [1, 0, 0]), 0.125)
    assert ids[0] == row[1] and t[0] == F(0.125)
    # tmin == tmax crosses nothing, also inside a sphere
    s = span(RS.rays([x0, -0.5, 0.0], [1, 0, 0], 0.05, 0.05))
    assert (s["count"], s["idEnter"], s["idExit"], s["length"], s["flags"]) == (0, -1, -1, 0, 0) and np.isposinf(s["tEnter"]) and np.isneginf(s["tExit"])
    # a negative tmin: the part of the row behind the origin
    s = span(RS.rays([x0 + 0.75, -0.5, 0.0], [1, 0, 0], -10.0, 0.0))               # from the fourth centre backwards
    assert s["count"] == 4 and s["length"] == 7 << 23 and s["tEnter"] == F(-0.875) and s["tExit"] == 0 and s["idEnter"] == row[0] and s["idExit"] == row[3]
    # a sphere touched only at t == tmax is not crossed; one more ulp of window and it is
    s = span(RS.rays([x0 - 3.0, -0.5, 0.0], [1, 0, 0], 0.0, 2.875))
    assert s["count"] == 0
    s = span(RS.rays([x0 - 3.0, -0.5, 0.0], [1, 0, 0], 0.0, float(np.nextafter(F(2.875), F(9)))))
    assert s["count"] == 1 and s["idEnter"] == row[0] == s["idExit"] and s["tEnter"] == F(2.875)
    # ... and one left behind exactly at t == tmin
    s = span(RS.rays([x0 + 0.125, -0.5, 0.0], [1, 0, 0], 0.0, 0.2))
    assert s["count"] == 1 and s["idEnter"] == row[1] and s["tEnter"] == 0 and s["tExit"] == F(0.2)
    # in units of the direction: nothing is normalised, and the length does not depend on |d|
    s = span(RS.rays([x0 - 3.0, -0.5, 0.0], [4, 0, 0]))
    assert s["count"] == 7 and s["length"] == 7 << 24 and s["tEnter"] == F(2.875 / 4)


def test_coincident_eight(pkg):
    rec, sp, same = RS.coincident(pkg)
    x = rec["pos"][same[0], :3]
    d = np.array([0.3, -0.2, 0.9], F)
    s = pkg.ray_spans_host(rec, sp, RS.rays(x - F(0.2) * d, d), 0.1)[0]             # through the common centre, from outside
    # (each of the eight gives the same q, a whole diameter up to the rounding of tca +- thc at |t| <= 0.4: 2 ulp(0.4) / 0.2 * 2^24 = 5)
    assert s["count"] >= 8 and s["idEnter"] == same.min() and s["length"] >= 8 * ((1 << 24) - 5)
    for variant in (0, 1):
        assert pkg.ray_spans_walk_host(rec, sp, RS.rays(x - F(0.2) * d, d), 0.1, variant=variant)[0].tobytes() == s.tobytes()


def test_clamped_records_are_never_counted(pkg):
    sp = RS.params(pkg)
    lo, dims, cs = RS.grid(pkg, sp)
    hi = lo + dims.astype(F) * cs
    pos = np.array([[0.25, -0.5, 0.125], [hi[0] + F(0.3), -0.5, 0.125], [lo[0] - F(0.01), -0.5, 0.125], [np.nan, -0.5, 0.125]], F)
    rec = records(pkg, pos, np.zeros_like(pos))
    r = np.concatenate([RS.rays([hi[0] + 2, -0.5, 0.125], [-1, 0, 0]), RS.rays([lo[0] - 2, -0.5, 0.125], [1, 0, 0])])
    for fn in (lambda rc: pkg.ray_spans_host(rc, sp, r, 0.25), lambda rc: pkg.ray_spans_walk_host(rc, sp, r, 0.25, variant=0),
               lambda rc: pkg.ray_spans_walk_host(rc, sp, r, 0.25, variant=1)):
        s = fn(rec)
        assert s["count"].tolist() == [1, 1] and s["idEnter"].tolist() == [0, 0] and s["idExit"].tolist() == [0, 0]
        # (a whole diameter up to the rounding of tca +- thc at |t| < 8: 2 * ulp(4) / 2 over 0.5, in 2^-24: 16, and the rounding of q)
        assert (np.abs(s["length"].astype(np.int64) - (1 << 24)) <= 17).all()
        s = fn(rec[1:])
        assert s["count"].tolist() == [0, 0] and (s["idEnter"] == -1).all() and (s["length"] == 0).all()
    # every scene with clamped records: no id of a row is a clamped record's
    name, rec, sp, casts = [sc for sc in _scenes(pkg) if sc[0] == "clamped records"][0]
    out = ~SR.takes_part(rec, RS.grid(pkg, sp))
    assert out.sum() > 100
    for r, radius, kw in casts:
        s = pkg.ray_spans_host(rec, sp, r, radius, **kw)
        hit = s["count"] > 0
        assert hit.any() and not out[s["idEnter"][hit]].any() and not out[s["idExit"][hit]].any()


def test_void_rays(pkg):
    from test_rays_cpu import VOID
    rec, sp = RS.uniform(pkg, 300, 41)
    r = np.array(VOID, F)
    r[:, 0:3] += rec["pos"][5, :3] - np.array([0.5, 0, 0], F)
    for fn in (lambda: pkg.ray_spans_host(rec, sp, r, 0.25, with_info=True), lambda: pkg.ray_spans_walk_host(rec, sp, r, 0.25, with_info=True, variant=0),
               lambda: pkg.ray_spans_walk_host(rec, sp, r, 0.25, with_info=True, variant=1)):
        s, info = fn()
        assert (s["flags"] == 1).all() and (s["count"] == 0).all() and (s["idEnter"] == -1).all() and (s["idExit"] == -1).all() and (s["length"] == 0).all()
        assert np.isposinf(s["tEnter"]).all() and np.isneginf(s["tExit"]).all()
        assert info.voidRays == len(r) and info.crossed == 0 and info.total == 0 and info.maxCount == 0
    good = RS.rays(rec["pos"][5, :3] - np.array([0.5, 0, 0], F), [1, 0, 0], 0.0, INF)
    s, info = pkg.ray_spans_host(rec, sp, good, 0.25, with_info=True)
    assert s["flags"][0] == 0 and s["count"][0] >= 1 and info.voidRays == 0 and info.crossed == 1


def test_info_sums_and_fluid_only(pkg):
    rec, sp = RS.with_ghosts(pkg)
    r = RS.void_mix(RS.segments(np.random.default_rng(5), sp, 2048), np.random.default_rng(6))
    ghost = rec["isGhost"] != 0
    s, info = pkg.ray_spans_host(rec, sp, r, 0.25, with_info=True)
    info_of_rows(s, info, "all records")
    assert info.voidRays > 0 and info.maxCount > 1 and info.flags == 0 and info.radius == F(0.25)
    sf, inf_ = pkg.ray_spans_host(rec, sp, r, 0.25, fluid_only=True, with_info=True)
    info_of_rows(sf, inf_, "fluid only")
    assert inf_.flags == pkg.SPH_RAYS_FLUID_ONLY and inf_.total < info.total
    hit = sf["count"] > 0
    assert not ghost[sf["idEnter"][hit]].any() and not ghost[sf["idExit"][hit]].any() and ghost[s["idEnter"][s["count"] > 0]].any()
    # the same as the spans of the fluid records alone
    keep = np.flatnonzero(~ghost)
    sk = pkg.ray_spans_host(rec[keep], sp, r, 0.25)
    for name in ("tEnter", "tExit", "count", "flags", "length"):
        assert sk[name].tobytes() == sf[name].tobytes(), name
    assert np.array_equal(np.where(sk["idEnter"] >= 0, keep[np.maximum(sk["idEnter"], 0)], -1), sf["idEnter"])
    # a ray that starts outside every sphere: tEnter / idEnter are the cast's t / id
    far = RS.segments(np.random.default_rng(7), sp, 1024, tmax=INF)
    far[:, 0:3] *= F(6.0)
    far[:, 4:7] = RS.box_cloud(np.random.default_rng(8), sp, 1024) - far[:, 0:3]
    t, ids, _, _ = pkg.rays_host(rec, sp, far, 0.25)
    s = pkg.ray_spans_host(rec, sp, far, 0.25)
    assert s["tEnter"].tobytes() == t.tobytes() and s["idEnter"].tobytes() == ids.tobytes() and (ids >= 0).sum() > 100


def test_first_entry_is_the_casts(pkg):
    """On rays that start outside every sphere with tmax = +inf (the `far` and `lat` families of every scene), tEnter / idEnter are the
    cast's t / id byte for byte -- ray_spans_ref.first_entry has the two exceptions the definitions leave and proves each ray's."""
    rays = 0
    for name, rec, sp, casts in _scenes(pkg):
        for r, radius, kw in casts:
            if not SR.far_or_lat(pkg, r):
                continue
            hits = pkg.rays_host(rec, sp, r, radius, **kw)
            SR.first_entry(pkg, rec, sp, r, radius, pkg.ray_spans_host(rec, sp, r, radius, **kw), hits, f"{name} r {radius}", exact=name == "uniform 1200")
            rays += len(r)
    assert rays > 5000


def test_thickness_per_unit_path(pkg):
    """What `length` means for a cloud: q is the share of the sphere's OWN chord that lies in the window, so a sphere crossed whole counts
    as one diameter whatever the impact parameter (a disc splat), and a line meets n pi r^2 spheres per unit path: the thickness per
    unit path is n * pi r^2 * 2 r, three halves of the packing fraction n * 4 pi r^3 / 3 (the mean chord of a sphere is 4 r / 3, not
    2 r).  1200 uniform records in the box of 4 x 3 x 3.5, 4096 segments that keep r away from its walls: about 11000 crossings, a
    Poisson count with a relative deviation of 1 %; asserted at five deviations."""
    rec, sp = RS.uniform(pkg, 1200, 42)
    rng = np.random.default_rng(21)
    radius = 0.125
    c, half = np.array(list(sp.param_boxCenter), F), np.array(list(sp.param_boxHalf), F) - F(radius)
    a = c + (rng.random((4096, 3)).astype(F) * 2 - 1) * half
    b = c + (rng.random((4096, 3)).astype(F) * 2 - 1) * half
    s = pkg.ray_spans_host(rec, sp, RS.rays(a, b - a, 0.0, 1.0), radius)
    path = np.linalg.norm((b - a).astype(np.float64), axis=1).sum()
    got = pkg.ray_thickness(s, radius).sum() / path
    density = 1200 / (4 * 3 * 3.5)
    want = density * np.pi * radius ** 2 * 2 * radius
    print("thickness per unit path", got, "n pi r^2 2 r", want, "packing fraction", density * 4 * np.pi * radius ** 3 / 3, "crossings", int(s["count"].sum()))
    assert abs(got / want - 1) < 0.05


def test_layouts(pkg, tmp_path):
    from support import c_layout
    size, offsets, _ = c_layout("SphRaySpan", pkg.SphRaySpan, [], tmp_path)
    assert size == 32 == pkg.RAY_SPAN_DTYPE.itemsize and offsets == [(n, pkg.RAY_SPAN_DTYPE.fields[n][1]) for n in FIELDS]
    assert [o for _, o in offsets] == [0, 4, 8, 12, 16, 20, 24]
    size, offsets, _ = c_layout("SphRaySpansInfo", pkg.SphRaySpansInfo, [], tmp_path)
    assert size == 48 == C.sizeof(pkg.SphRaySpansInfo) and offsets == [(n, getattr(pkg.SphRaySpansInfo, n).offset) for n, _ in pkg.SphRaySpansInfo._fields_]
    assert pkg.SPH_OPT_RAY_SPANS_VARIANT == 15


def test_refusals_and_empty_calls(pkg):
    L = pkg.load_library()
    rec, sp = RS.uniform(pkg, 300, 41)
    cs = float(RS.grid(pkg, sp)[2])
    r = RS.segments(np.random.default_rng(1), sp, 4)
    info = pkg.SphRaySpansInfo()
    vp = C.c_void_p
    rows = np.zeros(4, pkg.RAY_SPAN_DTYPE)
    for fn, extra in ((L.sph_rays_span_host, ()), (L.sph_rays_span_walk_host, (0,)), (L.sph_rays_span_walk_host, (1,))):
        call = lambda radius, flags=0, m=4, rp=r.ctypes.data_as(vp), pp=rec.ctypes.data_as(vp), out=C.byref(info), spp=C.byref(sp), rows_p=rows.ctypes.data_as(vp): \
            fn(pp, len(rec), spp, rp, m, radius, flags, *extra, rows_p, out)
        assert call(0.25) == 0 and info.rays == 4
        assert call(0.5 * cs) == 0                                                  # half a cell exactly is allowed
        for bad in (0.0, -0.1, float("nan"), float("inf"), float(np.nextafter(F(0.5 * cs), F(1)))):
            assert call(bad) == -1, bad
        assert call(0.25, flags=pkg.SPH_RAYS_ANY_HIT) == -1 and call(0.25, flags=4) == -1 and call(0.25, m=1 << 31) == -1
        assert call(0.25, rp=None) == -1 and call(0.25, pp=None) == -1 and call(0.25, out=None) == -1 and call(0.25, spp=None) == -1
        assert call(0.25, rows_p=None) == 0                                         # rows may be null
    for bad in (-1, 2):
        assert L.sph_rays_span_walk_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), r.ctypes.data_as(vp), 4, 0.25, 0, bad, None, C.byref(info)) == -1
    with pytest.raises(pkg.SphError):
        pkg.ray_spans_host(rec, sp, np.zeros((3, 7), F), 0.25)
    s, info = pkg.ray_spans_host(rec, sp, np.zeros((0, 8), F), 0.25, with_info=True)   # m = 0 and n = 0
    assert s.shape == (0,) and info.rays == 0 and info.crossed == 0
    for variant in (0, 1):
        s, info = pkg.ray_spans_walk_host(rec[:0], sp, r, 0.25, with_info=True, variant=variant)
        assert (s["count"] == 0).all() and (s["idEnter"] == -1).all() and info.rays == 4 and info.crossed == 0
