"""The fused neighbourhood reductions on the CPU: sph_aggregate_host (the C++ twin that runs the device's per-candidate functions over
HostGrid) against the independent numpy restatement aggregate_ref, byte for byte, on the query scenes; the float64 bound of the sums,
the counts, the order-independence of the extrema, signed zeros and NaN, the refusals and the struct layouts.  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import aggregate_ref as AR
from aggregate_ref import PARTICLE_CASES, QUERY_CASES, radius_of, same_bytes, values_for
import neighbors_ref as NR
import query_scenes as QS
from support import c_layout, records

F = np.float32
vp = C.c_void_p


def check_cases(pkg, rec, sp, cases, what, points=None, **kw):
    for op, weight, self_, delta, moments, fac, c in cases:
        x = values_for(len(rec), c)
        R = radius_of(sp, fac)
        args = dict(op=op, weight=weight, self_=self_, delta=delta, moments=moments, **kw)
        got = pkg.aggregate_host(rec, sp, x, R, points=points, counts=True, **args)
        want = AR.aggregate(pkg, rec, sp, x, R, points=points, **args)
        same_bytes(got, want, f"{what} {args} R {fac} h C {c}")


@pytest.mark.parametrize("seed", [21, 22])
def test_uniform(pkg, seed):
    rec, sp = QS.uniform(pkg, 1000, seed)
    check_cases(pkg, rec, sp, PARTICLE_CASES, f"uniform {seed}")


def test_lattice_with_exact_ties(pkg):
    rec, sp = QS.lattice(pkg)
    check_cases(pkg, rec, sp, PARTICLE_CASES, "lattice")


def test_coincident_particles(pkg):
    rec, sp, same = QS.coincident(pkg)
    check_cases(pkg, rec, sp, PARTICLE_CASES, "coincident")
    out, cnt = pkg.aggregate_host(rec, sp, np.ones(len(rec), F), 1.0, counts=True)
    assert (cnt[same] >= 7).all() and (out[same, 0] == cnt[same]).all()                 # the seven others at distance 0, never the own slot


@pytest.mark.parametrize("fluid_only", [False, True])
def test_ghosts(pkg, fluid_only):
    rec, sp = QS.with_ghosts(pkg)
    check_cases(pkg, rec, sp, PARTICLE_CASES, "ghosts", fluid_only=fluid_only)
    check_cases(pkg, rec, sp, QUERY_CASES[:4], "ghosts, query", points=rec["pos"][:333, :3], fluid_only=fluid_only)
    ghost = rec["isGhost"] != 0
    x = (~ghost).astype(F)                                                              # 1 on fluid records
    out, cnt = pkg.aggregate_host(rec, sp, x, radius_of(sp, 2.0), self_=True, fluid_only=fluid_only, counts=True)
    mx = pkg.aggregate_host(rec, sp, x, radius_of(sp, 2.0), op="max", self_=True, fluid_only=fluid_only)
    if fluid_only:
        assert (cnt[ghost] == 0).all() and (out[ghost] == 0).all() and np.isneginf(mx[ghost]).all()      # a ghost target: an empty row
        assert (out[~ghost, 0] == cnt[~ghost]).all()                                                       # no ghost among the candidates
    else:
        assert (cnt[ghost] > 0).all() and (out[:, 0] < cnt).any()


@pytest.mark.parametrize("crowd", [65, 200])
def test_crowded_cell(pkg, crowd):
    rec, sp, start, members = QS.crowded_cell(pkg, crowd)
    assert members >= crowd
    check_cases(pkg, rec, sp, PARTICLE_CASES, f"crowd {crowd}")


def test_query_cloud(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    assert len(pts) == 701 and not NR.inside_grid(pkg, rec["pos"], sp)
    check_cases(pkg, rec, sp, QUERY_CASES, "query cloud", points=pts)
    x = values_for(len(rec), 3)
    for op, empty in (("sum", 0.0), ("mean", 0.0), ("max", -np.inf), ("min", np.inf)):
        out, cnt = pkg.aggregate_host(rec, sp, x, radius_of(sp, 2.0), points=pts, op=op, counts=True)
        rows = [5, 256, 700]                                                            # the three non-finite points
        assert (cnt[rows] == 0).all() and (out[rows] == empty).all() and cnt.sum() > 0
        assert op == "max" or not np.signbit(out[rows]).any()                           # (+0, not -0)


def test_non_finite_particles_and_values(pkg):
    rec, sp = QS.uniform(pkg, 1000, 23)
    rec["pos"][7, 0] = np.nan
    rec["pos"][300, 2] = np.inf
    check_cases(pkg, rec, sp, PARTICLE_CASES, "non-finite positions")
    x = values_for(len(rec), 2)
    R = radius_of(sp, 2.0)
    out, cnt = pkg.aggregate_host(rec, sp, x, R, counts=True)
    assert cnt[7] == 0 and cnt[300] == 0 and (out[[7, 300]] == 0).all()
    out, cnt = pkg.aggregate_host(rec, sp, x, R, self_=True, counts=True)               # the own slot stays, by identity
    assert cnt[7] == 1 and cnt[300] == 1 and np.array_equal(out[[7, 300]], x[[7, 300]])
    # NaN and inf values reach the rows that accept them, and no other row
    clean = pkg.aggregate_host(rec, sp, x, R, op="mean", weight="poly6")
    x2 = x.copy()
    x2[11, 0], x2[12, 1] = np.nan, np.inf
    off, idx = pkg.neighbors_host(rec, sp, R)
    sees = lambda j: np.array([j in idx[off[i]:off[i + 1]] for i in range(len(rec))])
    dirty = pkg.aggregate_host(rec, sp, x2, R, op="mean", weight="poly6")
    assert np.isnan(dirty[sees(11), 0]).all() and np.isinf(dirty[sees(12), 1]).all()
    assert np.array_equal(dirty[~sees(11), 0].view(np.uint32), clean[~sees(11), 0].view(np.uint32))
    assert np.array_equal(dirty[~sees(12), 1].view(np.uint32), clean[~sees(12), 1].view(np.uint32))
    same_bytes(pkg.aggregate_host(rec, sp, x2, R, op="mean", weight="poly6", counts=True), AR.aggregate(pkg, rec, sp, x2, R, op="mean", weight="poly6"), "NaN values")


@pytest.mark.parametrize("op,weight", [("sum", "one"), ("sum", "poly6"), ("mean", "one"), ("mean", "poly6")])
def test_sums_within_the_float64_bound(pkg, op, weight):
    """SUM and MEAN against a float64 sum over the float64 brute-force pairs, within gamma_k * sum |w v| (over W for the mean), gamma_k =
    k u / (1 - k u), u = 2^-24, k = count + 2 (count + 3 for the mean): count products, count - 1 sums and, for the mean, as many sums of
    W and one division.  The weights enter the float64 sum as the fp32 numbers the definition rounds them to (w = 1 is exact): the bound
    is that of the accumulation, which is what the fused call adds to the definition."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    for fac, c in ((1.0, 3), (2.0, 5), (3.0, 1)):
        R = radius_of(sp, fac)
        x = values_for(len(rec), c)
        off, idx, margin = NR.brute_force(pkg, rec["pos"], sp, R)
        assert margin > 1e-6, "a pair so close to the radius that fp32 and float64 may disagree about it"
        got, cnt = pkg.aggregate_host(rec, sp, x, R, op=op, weight=weight, counts=True)
        assert np.array_equal(cnt, np.diff(off))
        rows, recv, send, d, r2 = AR.edges(pkg, rec, sp, R)
        assert np.array_equal(send, idx)                                                # the same pairs in the same order
        w = AR.weights(weight, R, r2).astype(np.float64)
        term = w[:, None] * x[send].astype(np.float64)
        s64, a64, W64 = np.zeros((rows, c)), np.zeros((rows, c)), np.zeros(rows)
        np.add.at(s64, recv, term)
        np.add.at(a64, recv, np.abs(term))
        np.add.at(W64, recv, w)
        k = cnt.astype(np.float64) + (3 if op == "mean" else 2)
        if op == "mean":
            ok = W64 > 0
            s64 = np.where(ok[:, None], s64 / np.where(ok, W64, 1.0)[:, None], 0.0)
            a64 = np.where(ok[:, None], a64 / np.where(ok, W64, 1.0)[:, None], 0.0)
        err, bound = np.abs(got.astype(np.float64) - s64), AR.gamma(k)[:, None] * a64
        print(f"{op} {weight} R {fac} h: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, mean count {cnt.mean():.1f}")
        assert (err <= bound).all()


def test_counts_are_the_count_only_degrees(pkg):
    rec, sp = QS.with_ghosts(pkg)
    x = values_for(len(rec), 1)
    for fac in (1.0, 2.0, 3.0):
        for self_ in (False, True):
            R = radius_of(sp, fac)
            deg = np.diff(pkg.neighbors_host(rec, sp, R, self_=self_, count_only=True)[0])
            for op in ("sum", "max"):
                assert np.array_equal(pkg.aggregate_host(rec, sp, x, R, op=op, self_=self_, counts=True)[1], deg)
    off, idx = pkg.neighbors_host(rec, sp, radius_of(sp, 2.0))
    ghost = rec["isGhost"] != 0
    fluid = np.add.reduceat(np.append(~ghost[idx], False).astype(np.int64), off[:-1]) * (np.diff(off) > 0)
    cnt = pkg.aggregate_host(rec, sp, x, radius_of(sp, 2.0), fluid_only=True, counts=True)[1]
    assert np.array_equal(cnt[~ghost], fluid[~ghost]) and (cnt[ghost] == 0).all()


def test_extrema_do_not_depend_on_the_particle_order(pkg):
    """MAX / MIN of a row are the same whatever ids the particles carry; a SUM follows the (cell, id) order and is not asserted to be."""
    rec, sp = QS.uniform(pkg, 1000, 21)
    x = values_for(len(rec), 5)
    x[::7] = x[3]                                                                       # equal values in many rows
    perm = np.random.default_rng(4).permutation(len(rec))
    R = radius_of(sp, 2.0)
    for op in ("max", "min"):
        for delta in (False, True):
            a = pkg.aggregate_host(rec, sp, x, R, op=op, delta=delta)
            b = pkg.aggregate_host(rec[perm], sp, x[perm], R, op=op, delta=delta)
            assert a[perm].tobytes() == b.tobytes(), (op, delta)
    a, b = pkg.aggregate_host(rec, sp, x, R), pkg.aggregate_host(rec[perm], sp, x[perm], R)
    assert np.allclose(a[perm], b, rtol=0, atol=1e-4)


def test_signed_zeros_and_nan_in_one_row(pkg):
    sp = QS.params(pkg)
    pos = np.array([[0.3, -0.45, 0.2], [0.35, -0.45, 0.2], [0.3, -0.4, 0.2], [0.3, -0.45, 0.25]], F)
    rec = records(pkg, pos, np.zeros_like(pos))
    for order in ([0.0, -0.0, np.nan], [-0.0, np.nan, 0.0], [np.nan, 0.0, -0.0]):
        x = np.array([5.0] + order, F)
        mx = pkg.aggregate_host(rec, sp, x, 0.5, op="max")
        mn = pkg.aggregate_host(rec, sp, x, 0.5, op="min")
        assert mx[0, 0] == 0 and not np.signbit(mx[0, 0]) and mn[0, 0] == 0 and np.signbit(mn[0, 0]), order
    only_nan = np.array([5.0, np.nan, np.nan, np.nan], F)
    out, cnt = pkg.aggregate_host(rec, sp, only_nan, 0.5, op="max", counts=True)
    assert cnt[0] == 3 and np.isneginf(out[0, 0])                                       # a NaN never wins, and is counted


def test_refusals_write_nothing(pkg):
    """Every SPH_ERR_ARG case of include/sph_abi.h but one: rows * planes * channels beyond size_t cannot be reached through a 64-bit
    size_t (rows <= 2^31 - 1 or the engine's particle limit, planes * channels <= 512); the check stays in the library."""
    L = pkg.load_library()
    rec, sp = QS.uniform(pkg, 50, 3)
    n, h = len(rec), sp.param_h
    x = values_for(n, 4)
    pts = np.zeros((3, 4), F)
    out, cnt = np.full((n, 4, 4), 7.0, F), np.full(n, 9, np.uint32)

    def call(cfg, points=None, m=0, values=x, out_=out, cnt_=cnt, params=sp, cfg_null=False):
        rc = L.sph_aggregate_host(rec.ctypes.data_as(vp), n, C.byref(params) if params is not None else None, None if cfg_null else C.byref(cfg),
                                  None if points is None else points.ctypes.data_as(vp), m, None if values is None else values.ctypes.data_as(vp),
                                  None if out_ is None else out_.ctypes.data_as(vp), None if cnt_ is None else cnt_.ctypes.data_as(vp))
        assert (out == 7.0).all() and (cnt == 9).all()
        return rc

    good = dict(radius=h, channels=4)
    assert call(pkg.aggregate_config(**good), cfg_null=True) == -1 and call(pkg.aggregate_config(**good), params=None) == -1
    assert call(pkg.aggregate_config(**good), values=None) == -1 and call(pkg.aggregate_config(**good), out_=None) == -1
    for R in (0.0, -1.0, float("nan"), float("inf"), 3.01 * h):
        assert call(pkg.aggregate_config(radius=R, channels=4)) == -1
    for bad in (dict(op=-1), dict(op=4), dict(weight=-1), dict(weight=2), dict(flags=16), dict(channels=0), dict(channels=129), dict(channels=-3),
                dict(op=pkg.SPH_AGGREGATE_MEAN, flags=pkg.SPH_AGGREGATE_MOMENTS), dict(op=pkg.SPH_AGGREGATE_MAX, flags=pkg.SPH_AGGREGATE_MOMENTS),
                dict(op=pkg.SPH_AGGREGATE_MAX, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6), dict(op=pkg.SPH_AGGREGATE_MIN, weight=pkg.SPH_AGGREGATE_WEIGHT_POLY6)):
        assert call(pkg.aggregate_config(**dict(good, **bad))) == -1, bad
    padded = pkg.aggregate_config(**good)
    padded.pad[1] = 1
    assert call(padded) == -1
    for flag in (pkg.SPH_AGGREGATE_SELF, pkg.SPH_AGGREGATE_DELTA):                      # particle targets only
        assert call(pkg.aggregate_config(flags=flag, **good), points=pts, m=3) == -1
    assert call(pkg.aggregate_config(**good), points=pts, m=1 << 31) == -1
    # an output that overlaps the values as address ranges
    both = np.full(n * 4 + 8, 7.0, F)
    vals, over = both[:n * 4], both[8:]
    rc = L.sph_aggregate_host(rec.ctypes.data_as(vp), n, C.byref(sp), C.byref(pkg.aggregate_config(**good)), None, 0, vals.ctypes.data_as(vp),
                              over.ctypes.data_as(vp), None)
    assert rc == -1 and (both == 7.0).all() and b"overlap" in L.sph_last_error()
    as_cnt = both[4:].view(np.uint32)
    assert L.sph_aggregate_host(rec.ctypes.data_as(vp), n, C.byref(sp), C.byref(pkg.aggregate_config(**good)), None, 0, vals.ctypes.data_as(vp),
                                out.ctypes.data_as(vp), as_cnt.ctypes.data_as(vp)) == -1 and (both == 7.0).all() and (out == 7.0).all()
    with pytest.raises(pkg.SphError):
        pkg.aggregate_host(rec, sp, x, h, op="median")
    with pytest.raises(pkg.SphError):
        pkg.aggregate_host(rec, sp, x[:-1], h)
    # the valid call writes; m = 0 and n = 0 succeed and write nothing
    assert call(pkg.aggregate_config(**good), points=pts, m=0) == 0
    none = np.zeros(0, pkg.PARTICLE_DTYPE)
    assert pkg.aggregate_host(none, sp, np.zeros((0, 4), F), h).shape == (0, 4)
    assert pkg.aggregate_host(none, sp, np.zeros((0, 4), F), h, points=np.zeros((5, 3), F), moments=True).shape == (5, 4, 4)
    assert pkg.aggregate_host(rec, sp, x, h, points=np.zeros((0, 3), F)).shape == (0, 4)


def test_default_config_and_layouts(pkg, tmp_path):
    cfg = pkg.aggregate_config()
    assert (cfg.radius, cfg.op, cfg.weight, cfg.flags, cfg.channels, list(cfg.pad)) == (0.0, 0, 0, 0, 1, [0, 0, 0])
    with pytest.raises(pkg.SphError):
        pkg.aggregate_config(pad=1)
    extra = ['printf("%d %d %d %d %d %d %d %d %d %d %d\\n", SPH_AGGREGATE_SUM, SPH_AGGREGATE_MEAN, SPH_AGGREGATE_MAX, SPH_AGGREGATE_MIN, '
             'SPH_AGGREGATE_WEIGHT_ONE, SPH_AGGREGATE_WEIGHT_POLY6, SPH_AGGREGATE_SELF, SPH_AGGREGATE_FLUID_ONLY, SPH_AGGREGATE_DELTA, '
             'SPH_AGGREGATE_MOMENTS, SPH_AGGREGATE_MAX_CHANNELS);', 'printf("%d\\n", SPH_OPT_AGGREGATE_VARIANT);']
    for name, kind in (("SphAggregateConfig", pkg.SphAggregateConfig), ("SphAggregateInfo", pkg.SphAggregateInfo)):
        size, offsets, rest = c_layout(name, kind, extra, tmp_path)
        assert size == C.sizeof(kind) == 32
        assert offsets == [(f, getattr(kind, f).offset) for f, _ in kind._fields_]
        assert [int(v) for v in rest[0].split()] == [pkg.SPH_AGGREGATE_SUM, pkg.SPH_AGGREGATE_MEAN, pkg.SPH_AGGREGATE_MAX, pkg.SPH_AGGREGATE_MIN,
                                                     pkg.SPH_AGGREGATE_WEIGHT_ONE, pkg.SPH_AGGREGATE_WEIGHT_POLY6, pkg.SPH_AGGREGATE_SELF,
                                                     pkg.SPH_AGGREGATE_FLUID_ONLY, pkg.SPH_AGGREGATE_DELTA, pkg.SPH_AGGREGATE_MOMENTS,
                                                     pkg.SPH_AGGREGATE_MAX_CHANNELS]
        assert int(rest[1]) == pkg.SPH_OPT_AGGREGATE_VARIANT
