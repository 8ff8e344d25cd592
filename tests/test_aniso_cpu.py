"""Anisotropic kernels on the CPU (sph_aniso_host, sph_aniso_lattice_host: the kernels' own sum, finish and node functions over the
counting sort of sph_neighbors_host) against the float64 restatement of aniso_ref.py (numpy.linalg.eigh): rows and lattice within
measured tolerances, what the ellipsoids are on a block, the degenerate neighbourhoods, the special records, the flatness of the
meshed level, and the argument errors.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import aniso_ref as AR
import aniso_scenes as AS
import neighbors_ref as NR
import query_scenes as QS
import sample_ref
import shell_scenes as SS

F = np.float32
DX = SS.DX
SCENES = ("block", "ball10", "ball5", "hole", "uniform")
# Four times the largest deviation of the twin from the float64 restatement over the five scenes (test_twin_against_float64 prints
# them): center in units of h, T = sum axisK axisK' per entry in units of support^2, amplitude relative.
TOL_CENTER, TOL_T, TOL_AMP = 4 * 6.6e-7, 4 * 2.2e-6, 4 * 2.5e-6
_CACHE = {}


def _scene(pkg, name):
    """(records, params, nominal or None, reference, (rows, info) of the twin) at the default config, computed once per session."""
    if name not in _CACHE:
        if name == "uniform":
            rec, sp = QS.uniform(pkg, 2000, seed=41)
            nominal = None
        else:
            rec, sp, nominal = dict(block=lambda: SS.block(pkg), ball10=lambda: SS.ball(pkg, 10.0), ball5=lambda: SS.ball(pkg, 5.0),
                                    hole=lambda: SS.hole(pkg))[name]()
        assert NR.inside_grid(pkg, rec["pos"], sp)
        h = float(F(sp.param_h))
        _CACHE[name] = (rec, sp, nominal, AR.rows(rec["pos"], rec["density"], 2.0 * h, h), pkg.aniso_host(rec, sp))
    return _CACHE[name]


def _well_formed(pkg, rows, info, n):
    assert rows.dtype == pkg.ANISO_DTYPE and rows.dtype.itemsize == 64 and len(rows) == n == info.rows and info.kind == 1
    valid = (rows["flags"] & pkg.SPH_ANISO_VALID) != 0
    assert (rows[~valid].view(np.uint8) == 0).all() and (rows["flags"] <= 7).all()
    sparse, clamped = (rows["flags"] & pkg.SPH_ANISO_SPARSE) != 0, (rows["flags"] & pkg.SPH_ANISO_CLAMPED) != 0
    assert not (sparse & clamped).any() and not (sparse & ~valid).any()
    assert info.numSparse == sparse.sum() and info.numClamped == clamped.sum() and info.maxCount == (rows["count"].max() if n else 0)
    assert info.maxReach == (rows["reach"].max() if n else 0) and (rows["count"][valid] >= 1).all()
    L = [np.linalg.norm(rows[k].astype(np.float64), axis=1) for k in ("axis0", "axis1", "axis2")]
    assert (L[0][valid] >= L[1][valid] * (1 - 1e-6)).all() and (L[1][valid] >= L[2][valid] * (1 - 1e-6)).all() and (L[2][valid] > 0).all()
    return valid, sparse, clamped, L


@pytest.mark.parametrize("name", SCENES)
def test_twin_against_float64(pkg, name):
    """count is exact; center, T = sum axisK axisK' and amplitude stay within four times the largest deviation measured over these five
    scenes (the factor covers other seeds).  Measured: center 6.6e-7 h (hole), T 2.2e-6 support^2 per entry (hole), amplitude 2.5e-6
    relative (ball10: 2.41e-6).  Flags agree except on the rows where a clamp decision (relative 1e-4) or minCount (a candidate on the sphere
    within rounding) is undecided on the reference; at these seeds no row of the five scenes is."""
    rec, sp, _, ref, (rows, info) = _scene(pkg, name)
    valid, sparse, clamped, _ = _well_formed(pkg, rows, info, len(rec))
    h = float(F(sp.param_h))
    assert np.array_equal(rows["count"].astype(np.int64), ref["count"]), "count is exact"
    assert np.array_equal(valid, ref["valid"])
    dc = np.abs(rows["center"].astype(np.float64) - ref["center"]).max() / h
    dT = np.abs(AR.twin_T(rows) - ref["T"]).max() / (h * h)
    amp = rows["amplitude"].astype(np.float64)
    dA = np.abs(amp - ref["amplitude"]).max() / np.abs(ref["amplitude"]).max() if len(rec) else 0.0
    rel = np.abs(amp - ref["amplitude"])[ref["amplitude"] > 0] / ref["amplitude"][ref["amplitude"] > 0]
    print(f"{name}: center {dc:.3g} h, T {dT:.3g} support^2, amplitude rel {rel.max():.3g}, undecided {ref['undecided'].mean():.2e}, "
          f"sparse {sparse.sum()} clamped {clamped.sum()} of {len(rec)}")
    assert dc <= TOL_CENTER and dT <= TOL_T and rel.max() <= TOL_AMP and dA <= TOL_AMP
    skip = ref["undecided"]
    assert skip.mean() <= 0.01, "fixture condition: too many rows at a decision"
    assert np.array_equal(rows["flags"][~skip].astype(np.int64), ref["flags"][~skip])
    assert abs(info.maxReach - ref["reach"].max()) <= 1e-5 * h and info.stencil == 2 and info.radius == F(2) * F(sp.param_h) and info.support == F(sp.param_h)


def test_jacobi_sweeps_through_the_twin(pkg):
    """The eigenvectors of the twin diagonalise the float64 covariance: over 28568 neighbourhoods (the five scenes, and the layer
    and the line with the clamps off, where the smallest eigenvalue is above 1e-6 of the largest), the largest off-diagonal of V' C V relative to the largest
    eigenvalue, V the normalised axes of the twin, is measured at 8.3e-7 (five sweeps; fp32 rounding of the covariance itself is of this
    size), and V' V differs from the identity by at most 2.8e-7.  The bounds asserted are 64 and 16 units of 2^-24: fifteen rotations of
    a few roundings each, and the cancellation in M / W - m m'."""
    worst_off, worst_orth, total = 0.0, 0.0, 0
    cases = [_scene(pkg, name)[:2] + (25,) for name in SCENES] + [AS.layer(pkg)[:2] + (25,), AS.line(pkg)[:2] + (4,)]
    for rec, sp, min_count in cases:
        h = float(F(sp.param_h))
        kw = dict(max_ratio=1e30, max_stretch=1e30, min_count=min_count)
        ref = AR.rows(rec["pos"], rec["density"], 2.0 * h, h, **kw)
        rows, info = pkg.aniso_host(rec, sp, **kw)
        use = ((rows["flags"] & pkg.SPH_ANISO_SPARSE) == 0) & (ref["raw"][:, 2] > 1e-3 * ref["raw"][:, 0])
        A = np.stack([rows["axis0"], rows["axis1"], rows["axis2"]], axis=1).astype(np.float64)[use]
        V = np.swapaxes(A / np.linalg.norm(A, axis=2, keepdims=True), 1, 2)
        D = np.einsum("iak,iab,ibl->ikl", V, ref["C"][use], V)
        off = np.abs(D - np.einsum("ikl,kl->ikl", D, np.eye(3))).max(axis=(1, 2)) / ref["raw"][use, 0] ** 2
        orth = np.abs(np.einsum("iak,ial->ikl", V, V) - np.eye(3)).max(axis=(1, 2))
        worst_off, worst_orth, total = max(worst_off, off.max()), max(worst_orth, orth.max()), total + int(use.sum())
    print(f"{total} neighbourhoods: off-diagonal of V' C V {worst_off:.3g}, V' V - I {worst_orth:.3g}")
    assert total > 3000 and worst_off <= 64 * 2.0 ** -24 and worst_orth <= 16 * 2.0 ** -24


def test_geometry_on_the_block(pkg):
    """20^3 particles at dx = h / 2.4, R = 2h, each statement on the float64 restatement and on the twin (prototype of the issue / the
    restatement here / the twin): deep particles (more than 6 dx below every face) have all s_k in [0.95, 1.05] (0.980 .. 1.015 /
    0.9802 .. 1.0154 / the same); particles of an outermost plane more than 6 dx from the other faces have |axis2| / |axis0| <= 0.75
    (largest 0.668, median 0.63 / 0.6675, 0.6285 / the same) and axis2 within |cos| >= 0.99 of the face normal (>= 0.999 / 0.99896 /
    0.99896); no row is sparse, the smallest count is 81; reachStencil is 2 and the largest reach 1.55 h (1.5528 h)."""
    rec, sp, nominal, ref, (rows, info) = _scene(pkg, "block")
    _, sparse, _, L = _well_formed(pkg, rows, info, len(rec))
    h = float(F(sp.param_h))
    dep, ax, _ = SS.depth(nominal, 20)
    deep = dep > 6.0
    others = np.sort(9.5 - np.abs(nominal), axis=1)
    face = (dep < 0.5) & (others[:, 1] > 6.0)
    assert deep.sum() == 6 ** 3 and face.sum() == 6 * 6 * 6
    views = (("float64", ref["s"], ref["axes"][:, 2]), ("twin", np.stack(L, axis=1) / h, rows["axis2"].astype(np.float64)))
    for who, s, a2 in views:
        ratio = s[face, 2] / s[face, 0]
        cos = np.abs(a2[face][np.arange(face.sum()), ax[face]]) / np.linalg.norm(a2[face], axis=1)
        print(f"block, {who}: deep s {s[deep].min():.4f} .. {s[deep].max():.4f}, face ratio max {ratio.max():.4f} median {np.median(ratio):.4f}, "
              f"cos min {cos.min():.5f}")
        assert s[deep].min() >= 0.95 and s[deep].max() <= 1.05, who
        assert ratio.max() <= 0.75, who
        assert cos.min() >= 0.99, who
    assert not sparse.any() and not (ref["flags"] & AR.SPARSE).any()
    assert rows["count"].min() == 81 == ref["count"].min()
    print(f"block: reach max {info.maxReach / h:.4f} h (float64 {ref['reach'].max() / h:.4f} h), reachStencil {info.reachStencil}")
    assert info.reachStencil == 2 and abs(info.maxReach / h - 1.55) < 0.01 and abs(ref["reach"].max() / h - 1.55) < 0.01


def test_limits_layer_and_line(pkg):
    """One jittered layer of 24 x 24: the interior rows (more than 6 dx from the rim) are clamped, |axis2| * maxRatio == |axis0| to
    rounding and axis2 lies along the plane's normal.  A line of 40 (minCount 4: a line has about 9 neighbours within 2h): both minor
    axes sit at the floor |axis0| / maxRatio."""
    rec, sp, nominal = AS.layer(pkg)
    rows, info = pkg.aniso_host(rec, sp)
    _, sparse, clamped, L = _well_formed(pkg, rows, info, len(rec))
    inner = (np.abs(nominal[:, :2]) < 11.5 - 6.0).all(axis=1)
    assert inner.sum() >= 100 and clamped[inner].all() and not sparse[inner].any()
    assert np.allclose(L[2][inner] * 4.0, L[0][inner], rtol=4 * 2.0 ** -24, atol=0)
    a2 = rows["axis2"][inner].astype(np.float64)
    cos = np.abs(a2[:, 2]) / L[2][inner]
    print(f"layer: |axis0| / h {L[0][inner].min() / 0.28:.3f} .. {L[0][inner].max() / 0.28:.3f}, cos min {cos.min():.5f}")
    assert cos.min() > 0.99
    rec, sp, nominal = AS.line(pkg)
    rows, info = pkg.aniso_host(rec, sp, min_count=4)
    _, sparse, clamped, L = _well_formed(pkg, rows, info, len(rec))
    assert not sparse.any() and clamped.all()
    for k in (1, 2):
        assert np.allclose(L[k] * 4.0, L[0], rtol=4 * 2.0 ** -24, atol=0)
    assert (np.abs(rows["axis0"][:, 0]) / L[0] > 0.99).all()
    assert pkg.aniso_host(rec, sp)[1].numSparse == len(rec)                        # (at the default minCount every row of the line is sparse)


def test_limits_few_lone_and_empty(pkg):
    """Two or three particles: sparse, the axes exactly support * sparseScale times the coordinate axes.  A lone particle: count 1.
    n = 0: empty rows."""
    for count in (2, 3):
        rec, sp = AS.few(pkg, count)
        rows, info = pkg.aniso_host(rec, sp, sparse_scale=0.75)
        _well_formed(pkg, rows, info, count)
        want = F(sp.param_h) * F(0.75)
        assert (rows["flags"] == (pkg.SPH_ANISO_VALID | pkg.SPH_ANISO_SPARSE)).all() and (rows["count"] == count).all() and info.numSparse == count
        for k, key in enumerate(("axis0", "axis1", "axis2")):
            assert (rows[key] == want * np.eye(3, dtype=F)[k]).all(), key
        ref = AR.rows(rec["pos"], rec["density"], 2 * 0.28, 0.28, sparse_scale=0.75)
        assert np.allclose(rows["center"], ref["center"], atol=1e-6) and np.allclose(rows["amplitude"], ref["amplitude"], rtol=1e-5)
    rec, sp = AS.few(pkg, 1)
    rows, info = pkg.aniso_host(rec, sp)
    assert rows["count"].tolist() == [1] and rows["flags"].tolist() == [3] and (rows["center"] == rec["pos"][:, :3]).all()
    assert rows["reach"][0] == F(sp.param_h) * F(0.5) and (info.maxCount, info.numSparse, info.reachStencil) == (1, 1, 1)
    rows, info = pkg.aniso_host(np.zeros(0, pkg.PARTICLE_DTYPE), sp)
    assert len(rows) == 0 and (info.rows, info.numSparse, info.maxCount, info.maxReach, info.reachStencil, info.kind) == (0, 0, 0, 0.0, 0, 1)
    vals, info = pkg.aniso_lattice_host(np.zeros(0, pkg.PARTICLE_DTYPE), sp, (0, 0, 0), 0.1, (3, 2, 2))
    assert vals.shape == (2, 2, 3) and (vals == 0).all()
    vals, info = pkg.aniso_lattice_host(rec, sp, (0, 0, 0), 0.1, (3, 0, 2))         # an empty lattice
    assert vals.size == 0 and info.rows == 1


def test_coincident_ghosts_and_non_finite(pkg):
    rec, sp, same = QS.coincident(pkg)
    rows, info = pkg.aniso_host(rec, sp)
    _well_formed(pkg, rows, info, len(rec))
    assert len({rows[i].tobytes() for i in same}) == 1, "coincident particles have identical rows"
    # ghosts: candidates like any other, unless FLUID_ONLY
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    a, ainfo = pkg.aniso_host(rec, sp)
    b, binfo = pkg.aniso_host(rec, sp, fluid_only=True)
    _well_formed(pkg, a, ainfo, len(rec))
    _well_formed(pkg, b, binfo, len(rec))
    assert (b[ghost].view(np.uint8) == 0).all() and binfo.flags == pkg.SPH_ANISO_FLUID_ONLY and ainfo.flags == 0
    assert (a["count"][ghost] > 0).all() and (b["count"][~ghost] < a["count"][~ghost]).any()
    assert b[~ghost].tobytes() == pkg.aniso_host(rec[~ghost], sp)[0].tobytes()     # FLUID_ONLY rows of the fluid = the rows of the fluid alone
    ref = AR.rows(rec["pos"], rec["density"], 1.0, 0.5, exclude=ghost)
    assert np.array_equal(b["count"].astype(np.int64), ref["count"])
    # a non-finite particle: an all-zero row, a candidate of nobody
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    base = pkg.aniso_host(np.delete(rec, [7, 300]), sp)[0]
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    rows, info = pkg.aniso_host(rec, sp)
    _well_formed(pkg, rows, info, len(rec))
    assert (rows[[7, 300]].view(np.uint8) == 0).all() and np.delete(rows, [7, 300]).tobytes() == base.tobytes()
    # density <= 0: amplitude 0, the ellipsoid as ever
    rec, sp = QS.uniform(pkg, 500, seed=3)
    want = pkg.aniso_host(rec, sp)[0]
    rec["density"][10] = 0.0
    rec["density"][11] = -5.0
    rows = pkg.aniso_host(rec, sp)[0]
    assert (rows["amplitude"][[10, 11]] == 0).all() and rows["axis0"].tobytes() == want["axis0"].tobytes()


def test_lattice_against_float64(pkg):
    """The ball of 5 spacings, lattices of spacing h / 2: the cube of +-7 dx and the bar that overhangs the grid.  The twin stays within
    four times the largest deviation measured here, 3.5e-7 in units of the largest value (cube 3.5e-7, bar 3.3e-7; the scene is dense, the
    values run up to 21.6)."""
    rec, sp, _, ref, (rows, info) = _scene(pkg, "ball5")
    for overhang in (False, True):
        origin, spacing, dims = AS.ball_lattice(pkg, sp, overhang)
        vals, linfo = pkg.aniso_lattice_host(rec, sp, origin, spacing, dims)
        want = AR.lattice(ref, sp.param_mass, origin, spacing, dims)
        assert vals.shape == want.shape == dims[::-1] and vals.dtype == F and linfo.maxReach == info.maxReach
        dev = np.abs(vals - want).max() / want.max()
        print(f"lattice overhang {overhang}: dims {dims}, max {want.max():.4f}, nonzero {np.count_nonzero(vals)}, deviation {dev:.3g} of the largest value")
        assert want.max() > 0.9 and np.count_nonzero(vals) > 200 and dev <= 4 * 3.5e-7
        assert ((vals == 0) == (want == 0)).mean() > 0.995
    g = pkg.compute_grid_extents(sp)
    assert origin[0] < g.gridMin[0] - g.cellSize, "the bar starts outside the grid"


def test_lattice_equals_the_fraction(pkg):
    """With minCount 2^32 - 1, sparseScale 1, smoothing 0 and support h every ellipsoid is the sphere of radius h: the lattice is
    SPH_FIELD_FRACTION (sample_ref.brute in float64) within the same kind of bound: four times the 2.6e-7 of the largest value measured here."""
    rec, sp, _, _, _ = _scene(pkg, "ball5")
    origin, spacing, dims = AS.ball_lattice(pkg, sp)
    vals, info = pkg.aniso_lattice_host(rec, sp, origin, spacing, dims, min_count=2 ** 32 - 1, sparse_scale=1.0, smoothing=0.0, support=sp.param_h)
    assert info.numSparse == len(rec) and info.maxReach == F(sp.param_h) and info.reachStencil == 1
    ax = [(F(origin[k]) + np.arange(dims[k], dtype=F) * F(spacing[k])).astype(F) for k in range(3)]
    pts = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]
    want = sample_ref.brute(rec, pts, sp.param_h, sp.param_mass)["fraction"].reshape(vals.shape)
    dev = np.abs(vals - want).max() / want.max()
    print(f"fraction: max {want.max():.4f}, deviation {dev:.3g} of the largest value")
    assert want.max() > 0.9 and dev <= 4 * 2.6e-7


def test_three_cell_refusal(pkg):
    rec, sp, _, _, _ = _scene(pkg, "block")
    with pytest.raises(pkg.SphError, match="-1.*maxReach"):
        pkg.aniso_lattice_host(rec, sp, (0, 0, 0), 0.1, (2, 2, 2), support=3.1 * sp.param_h)
    rows, info = pkg.aniso_host(rec, sp, support=3.1 * sp.param_h)                 # the rows themselves are fine
    assert info.reachStencil == 0 and info.maxReach > 3 * sp.param_h and len(rows) == len(rec)


def test_flatness_of_the_meshed_level(pkg):
    """The purpose of the feature.  On the block's +z face, the height at which the field falls through half its bulk value, over 17 x
    17 columns within +-4 dx of the axis (nodes every dx / 8): the standard deviation of those heights for the twin's anisotropic
    lattice against that for the isotropic fraction (sample_ref.brute).  Prototype of the issue: 0.0427 dx against 0.0614 dx, ratio
    0.70.  Measured here through the twin: 0.0429 dx against 0.0618 dx, ratio 0.693.  Asserted: below the midpoint between the measured
    ratio and 1, 0.8465."""
    rec, sp, _, _, _ = _scene(pkg, "block")
    origin, spacing, dims, zs = AS.face_lattice()
    aniso = pkg.aniso_lattice_host(rec, sp, origin, spacing, dims)[0]
    ax = [(F(origin[k]) + np.arange(dims[k], dtype=F) * F(spacing[k])).astype(F) for k in range(3)]
    pts = np.stack(np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]
    iso = sample_ref.brute(rec, pts, sp.param_h, sp.param_mass)["fraction"].reshape(aniso.shape)
    core = (F(-2 * DX), F(-2 * DX), F(-2 * DX)), DX, (5, 5, 5)                      # the bulk value: 125 nodes around the block's centre
    cax = np.arange(5, dtype=F) * F(DX) + F(-2 * DX)
    cpts = np.stack(np.meshgrid(cax, cax, cax, indexing="ij"), axis=-1).reshape(-1, 3)
    bulk_a = float(pkg.aniso_lattice_host(rec, sp, *core)[0].mean())
    bulk_i = float(sample_ref.brute(rec, cpts, sp.param_h, sp.param_mass)["fraction"].mean())
    ha, hi = AR.level_heights(aniso, zs, 0.5 * bulk_a), AR.level_heights(iso, zs, 0.5 * bulk_i)
    assert np.isfinite(ha).all() and np.isfinite(hi).all()
    sa, si = ha.std(), hi.std()
    print(f"flatness: bulk {bulk_a:.4f} / {bulk_i:.4f}, mean height {ha.mean():.3f} / {hi.mean():.3f} dx, std {sa:.4f} dx against {si:.4f} dx, ratio {sa / si:.3f}")
    assert sa / si < 0.5 * (0.693 + 1.0)


def test_argument_errors_and_layout(pkg, tmp_path):
    from support import c_layout
    rec, sp = QS.uniform(pkg, 50, seed=1)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(radius=nan), dict(radius=inf), dict(radius=3.01 * sp.param_h), dict(support=nan), dict(support=inf), dict(smoothing=-0.1),
               dict(smoothing=1.1), dict(smoothing=nan), dict(max_ratio=0.9), dict(max_ratio=inf), dict(max_ratio=nan), dict(max_stretch=0.0),
               dict(max_stretch=inf), dict(max_stretch=nan), dict(sparse_scale=0.0), dict(sparse_scale=-1.0), dict(sparse_scale=inf), dict(sparse_scale=nan)):
        with pytest.raises(pkg.SphError, match="-1"):
            pkg.aniso_host(rec, sp, **kw)
        with pytest.raises(pkg.SphError, match="-1"):
            pkg.aniso_lattice_host(rec, sp, (0, 0, 0), 0.1, (2, 2, 2), **kw)
    for origin, spacing, dims in (((0, 0, 0), 0.0, (2, 2, 2)), ((0, 0, 0), nan, (2, 2, 2)), ((0, 0, 0), 0.1, (2, -1, 2)), ((0, 0, 0), 0.1, (2048, 2048, 2048))):
        with pytest.raises(pkg.SphError, match="-1"):
            pkg.aniso_lattice_host(rec, sp, origin, spacing, dims)
    L = pkg.load_library()
    info = pkg.SphAnisoInfo()
    vp = C.c_void_p
    cfg = pkg.aniso_config(flags=2)
    assert L.sph_aniso_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), C.byref(cfg), None, C.byref(info)) == -1
    cfg = pkg.aniso_config()
    assert (cfg.radius, cfg.support, cfg.maxRatio, cfg.maxStretch, cfg.sparseScale, cfg.minCount, cfg.flags) == (0.0, 0.0, 4.0, 1.5, 0.5, 25, 0)
    assert cfg.smoothing == F(0.9)
    assert L.sph_aniso_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), C.byref(cfg), None, C.byref(info)) == 0 and info.rows == 50
    assert L.sph_aniso_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), None, None, C.byref(info)) == -1
    assert L.sph_aniso_host(rec.ctypes.data_as(vp), len(rec), C.byref(sp), C.byref(cfg), None, None) == -1
    assert L.sph_aniso_host(None, len(rec), C.byref(sp), C.byref(cfg), None, C.byref(info)) == -1
    with pytest.raises(pkg.SphError, match="no field"):
        pkg.aniso_config(nothing=1)
    # defaults: radius None / <= 0 is 2 param_h, support None / <= 0 is param_h
    a = pkg.aniso_host(rec, sp)
    b = pkg.aniso_host(rec, sp, radius=2.0 * sp.param_h, support=sp.param_h)
    assert a[0].tobytes() == b[0].tobytes() and a[1].radius == F(2) * F(sp.param_h) and pkg.aniso_host(rec, sp, radius=-1.0, support=-1.0)[0].tobytes() == a[0].tobytes()
    for name, struct, size in (("SphAniso", pkg.SphAniso, 64), ("SphAnisoConfig", pkg.SphAnisoConfig, 32), ("SphAnisoInfo", pkg.SphAnisoInfo, 56)):
        got, offsets, _ = c_layout(name, struct, [], tmp_path)
        assert got == size == C.sizeof(struct) and offsets == [(f, getattr(struct, f).offset) for f, _ in struct._fields_]
