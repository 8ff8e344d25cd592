"""Active scalars without a GPU: the host twin sph_scalars_couple_host against the numpy restatement
tests/coupling_ref.py, bit for bit, the refusals by name, the facts that follow from the contract (RELAX never overshoots, a zero
buoyancy sum writes nothing), and the sign of the kick on the settled pool with the CPU oracle.

Bounds.  Books: the terms (double)c' - (double)c are exactly defined, only the order of their fp64 sum is free; the twin sums in index
order, the restatement with math.fsum, so they differ by at most coupling_ref.books_bound = 2 (n - 1) 2^-53 sum |t_i|."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import coupling_ref as CR
import obstacle_ref as R
import support
from support import same_bits

F = np.float32


def _bodies(pkg, c, E):
    """A rotated, spinning box and a sphere around the fluid block's centre c (extent E)."""
    return pkg.obstacle_array([pkg.obstacle(R.BOX, c + F(0.1 * E) * np.array([1, 0, -1], F), (0.15 * E, 0.1 * E, 0.12 * E), rotation=(0.8, 0.3, -0.4, 0.2),
                                            omega=(0.0, 3.0, 1.0)),
                               pkg.obstacle(R.SPHERE, c - F(0.2 * E) * np.array([1, 1, 0], F), 0.1 * E)])


def _normalised(arr):
    """The poses as the engine holds them after a set (the host functions use the rotation as given)."""
    return R.to_array(R.bodies(arr, normalise=True))


def _sources(pkg, c, E, K):
    """Both shapes, both modes, the world frame and both body frames, two overlapping sources on channel 0 (the order shows), the last
    channel fed too."""
    last = K - 1
    return [pkg.scalar_source(pkg.SPH_SOURCE_BOX, c - F(0.3 * E) * np.array([0, 1, 0], F), (0.6 * E, 0.12 * E, 0.6 * E), channel=0,
                              mode=pkg.SPH_SOURCE_RELAX, rate=40.0, target=2.5),
            pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.3 * E, channel=0, mode=pkg.SPH_SOURCE_RATE, rate=3.0),
            pkg.scalar_source(pkg.SPH_SOURCE_BOX, c, (0.25 * E, 0.5 * E, 0.1 * E), channel=0, mode=pkg.SPH_SOURCE_RELAX, rate=1e9, target=-1.0),
            pkg.scalar_source(pkg.SPH_SOURCE_BOX, (0.0, 0.05 * E, 0.0), (0.25 * E, 0.2 * E, 0.22 * E), channel=last, mode=pkg.SPH_SOURCE_RATE,
                              rate=7.0, body=0),
            pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, (0.02 * E, 0.0, 0.0), 0.2 * E, channel=last, mode=pkg.SPH_SOURCE_RELAX, rate=100.0,
                              target=0.25, body=1)]


def _state(pkg, seed=7):
    """scene4096 after 10 substeps with ghosts, non-finite positions and non-finite values mixed in."""
    rec = np.load(os.path.join(support.G, "scene4096.npz"))["after_10"].copy()
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    c, E = support.fluid_block(rec)
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(rec))
    rec["isGhost"][pick[:60]] = 1
    rec["isGhost"][pick[60:90]] = 2
    rec["pos"][pick[90:100], 0] = np.nan
    rec["pos"][pick[100:110], 2] = np.inf
    return rec, sp, c, E, pick


def _values(n, K, pick, seed=11):
    v = np.random.default_rng(seed).uniform(-1.0, 2.0, (n, K)).astype(F)
    v[pick[110:130], 0] = np.nan
    v[pick[130:140], K - 1] = np.inf
    v[pick[140:150], 0] = -np.inf
    return v


def _check_books(got_sums, got_hits, books, what):
    bound = CR.books_bound(books["hits"], books["abs_sum"])
    err = np.abs(got_sums - books["sums"])
    print(f"{what}: hits {books['hits'].tolist()} max err {err.max() if len(err) else 0:.3g} max bound {bound.max() if len(bound) else 0:.3g}")
    assert got_hits.tolist() == books["hits"].tolist(), what
    assert (err <= bound).all(), f"{what}: |got - reference| {err} above {bound}"


@pytest.mark.parametrize("K", [1, 4])
def test_host_twin_equals_the_restatement(pkg, K):
    rec, sp, c, E, pick = _state(pkg)
    values = _values(len(rec), K, pick)
    arr = _normalised(_bodies(pkg, c, E))
    src = _sources(pkg, c, E, K)
    beta = np.linspace(0.5, -0.25, K).astype(F)
    ref = np.linspace(0.1, 0.4, K).astype(F)
    g = (sp.param_gravityX, sp.param_gravityY, sp.param_gravityZ)
    dt = F(sp.param_timeStep)
    bodies = R.bodies(arr, normalise=False)
    sa = pkg.source_array(src).view(CR.SOURCE_DTYPE)
    for what, kw, rkw in (("sources and buoyancy", dict(beta=beta, ref=ref, sources=src, obstacles=arr), dict(beta=beta, ref=ref, sources=sa, bodies=bodies)),
                          ("sources alone", dict(sources=src, obstacles=arr), dict(sources=sa, bodies=bodies)),
                          ("buoyancy alone", dict(beta=beta, ref=ref), dict(beta=beta, ref=ref)),
                          ("reversed order", dict(sources=src[::-1], obstacles=arr), dict(sources=sa[::-1], bodies=bodies))):
        got_rec, got_c, sums, hits = pkg.scalars_couple_host(rec, sp, values, **kw)
        want_rec, want_c, books = CR.couple(rec, values, dt, g, **rkw)
        assert_records_equal(got_rec, want_rec, f"K={K} {what}")
        same_bits(got_c, want_c, f"K={K} {what}: values")
        _check_books(sums, hits, books, f"K={K} {what}")
        if "sources" in kw:
            assert (books["hits"] > 20).all(), books["hits"]                # every source acts, in both frames
        else:
            assert len(sums) == 0
        # records that are no targets keep their bits and their values
        off = ~CR.targets(rec)
        assert off.sum() >= 100 and got_rec[off].tobytes() == rec[off].tobytes()
        same_bits(got_c[off], values[off], "values of ghosts and of records with a non-finite position")
        bad = ~np.isfinite(values)
        assert got_c[bad].tobytes() == values[bad].tobytes()                # a non-finite value is never a hit
        if "beta" not in kw:
            assert_records_equal(got_rec, rec, "sources alone never change a record")
    # the order shows: the two overlapping sources on channel 0 do not commute
    a = pkg.scalars_couple_host(rec, sp, values, sources=src, obstacles=arr)[1]
    b = pkg.scalars_couple_host(rec, sp, values, sources=src[::-1], obstacles=arr)[1]
    fin = np.isfinite(a[:, 0]) & np.isfinite(b[:, 0])
    assert (a[fin, 0] != b[fin, 0]).sum() > 20
    # param_pause: nothing happens and nothing is counted; dt > 0 overrides param_timeStep
    paused = pkg.default_params()
    C.memmove(C.byref(paused), C.byref(sp), C.sizeof(sp))
    paused.param_pause = 1
    got_rec, got_c, sums, hits = pkg.scalars_couple_host(rec, paused, values, beta=beta, ref=ref, sources=src, obstacles=arr)
    assert_records_equal(got_rec, rec, "param_pause")
    same_bits(got_c, values, "param_pause: values")
    assert not sums.any() and not hits.any()
    got = pkg.scalars_couple_host(rec, sp, values, beta=beta, ref=ref, sources=src, obstacles=arr, dt=0.001)
    want = CR.couple(rec, values, F(0.001), g, beta=beta, ref=ref, sources=sa, bodies=bodies)
    assert_records_equal(got[0], want[0], "override dt")
    same_bits(got[1], want[1], "override dt: values")


def test_inside_is_strict(pkg):
    """A particle exactly on the sphere or on a face of the box is not inside; one a float below is."""
    sp = pkg.default_params()
    pos = np.array([[0.75, 0.5, -0.75], [0.75 - 2.0 ** -20, 0.5, -0.75], [2.0, 1.5, 0.0], [2.0, np.nextafter(F(1.5), F(0)), 0.0]], F)
    rec = support.records(pkg, pos, np.zeros_like(pos))
    src = [pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, (0.25, 0.5, -0.75), 0.5, rate=1.0),
           pkg.scalar_source(pkg.SPH_SOURCE_BOX, (2.0, 1.0, 0.0), (0.25, 0.5, 0.25), rate=1.0)]
    _, c, sums, hits = pkg.scalars_couple_host(rec, sp, np.zeros(4, F), sources=src)
    assert hits.tolist() == [1, 1] and (c[:, 0] != 0).tolist() == [False, True, False, True]
    want = CR.couple(rec, np.zeros(4, F), F(sp.param_timeStep), (0, -980, 0), sources=pkg.source_array(src).view(CR.SOURCE_DTYPE))
    same_bits(c, want[1], "strictness")


def test_relax_never_leaves_the_interval(pkg):
    rec, sp, c, E, pick = _state(pkg)
    rng = np.random.default_rng(5)
    everywhere = dict(shape=pkg.SPH_SOURCE_BOX, center=c, size=(2 * E, 2 * E, 2 * E), mode=pkg.SPH_SOURCE_RELAX)
    tgt = CR.targets(rec)
    for rate, target, dt in ((0.0, 1.0, 0.004), (3.0, 0.7, 0.004), (249.9, -2.0, 0.004), (250.0, 1e-3, 0.004), (1e30, 5.0, 0.004), (3.4e38, -1e30, 10.0),
                             (77.0, 0.0, 0.013)):
        values = (rng.standard_normal(len(rec)) * rng.choice([1e-6, 1.0, 1e6], len(rec))).astype(F)
        _, got, sums, hits = pkg.scalars_couple_host(rec, sp, values, sources=[pkg.scalar_source(rate=rate, target=target, **everywhere)], dt=dt)
        got, t = got[:, 0], F(target)
        assert hits[0] == tgt.sum()
        assert (got[tgt] >= np.minimum(values[tgt], t)).all() and (got[tgt] <= np.maximum(values[tgt], t)).all(), (rate, target)
        if float(F(dt)) * float(F(rate)) >= 1:
            # a = 1: c + fl(target - c) misses the target by the rounding of the subtraction (at most 2^-24 (|c| + |target|)) and that of
            # the addition (2^-24 of a number within the first error of the target): below 4 * 2^-24 max(|c|, |target|), on the inner side
            assert (np.abs(got[tgt].astype(np.float64) - float(t)) <= 2.0 ** -22 * np.maximum(np.abs(values[tgt]), abs(float(t)))).all()


def test_zero_buoyancy_sum_leaves_the_velocity_bits_alone(pkg):
    rec, sp, c, E, pick = _state(pkg)
    rec["vel"][::3, 0] = -0.0
    rec["vel"][::5, 1] = -0.0
    rec["vel"][::7, :3] = -0.0
    values = np.full((len(rec), 2), 0.5, F)
    values[1::2, 1] = 0.75
    # s = beta_0 (c_0 - ref_0) + beta_1 (c_1 - ref_1): exactly 0 where c_1 = 0.5, not where c_1 = 0.75; and 0 for beta = 0
    got, _, _, _ = pkg.scalars_couple_host(rec, sp, values, beta=(1.0, -2.0), ref=(0.25, 0.375))
    still = np.ones(len(rec), bool)
    still[1::2] = False
    assert got[still].tobytes() == rec[still].tobytes()
    moved = ~still & CR.targets(rec)
    assert (got["vel"][moved, 1] != rec["vel"][moved, 1]).all()
    assert_records_equal(got, CR.couple(rec, values, F(sp.param_timeStep), (0.0, -980.0, 0.0), beta=(1.0, -2.0), ref=(0.25, 0.375))[0], "kick")
    got, _, _, _ = pkg.scalars_couple_host(rec, sp, values, beta=(0.0, 0.0), ref=(3.0, 4.0))
    assert_records_equal(got, rec, "beta = 0")
    # a non-finite sum writes nothing either
    values[:, 0] = np.inf
    got, _, _, _ = pkg.scalars_couple_host(rec, sp, values, beta=(1.0, 0.0), ref=(0.0, 0.0))
    assert_records_equal(got, rec, "s = inf")


def test_every_refusal_by_name(pkg):
    rec, sp, c, E, pick = _state(pkg)
    values = np.zeros((len(rec), 2), F)
    arr = _normalised(_bodies(pkg, c, E))
    ok = dict(shape=pkg.SPH_SOURCE_BOX, center=c, size=(1.0, 1.0, 1.0), channel=1, mode=pkg.SPH_SOURCE_RELAX, rate=1.0, target=1.0, body=1)
    pkg.scalars_couple_host(rec, sp, values, sources=[pkg.scalar_source(**ok)], obstacles=arr)

    def refused(code, **kw):
        with pytest.raises(pkg.SphError, match=f"error {code}:"):
            pkg.scalars_couple_host(rec, sp, values, **kw)

    def bad(**change):
        return [pkg.scalar_source(**dict(ok, **change))]

    for change in (dict(shape=2), dict(shape=-1), dict(mode=2), dict(mode=-1), dict(channel=2), dict(channel=-1), dict(rate=-1.0), dict(rate=np.nan),
                   dict(rate=np.inf), dict(target=np.nan), dict(center=(np.inf, 0.0, 0.0)), dict(size=(1.0, np.nan, 1.0)), dict(size=(1.0, 0.0, 1.0)),
                   dict(size=(1.0, 1.0, -2.0)), dict(shape=pkg.SPH_SOURCE_SPHERE, size=(0.0, 1.0, 1.0)), dict(body=-2), dict(body=pkg.SPH_MAX_OBSTACLES)):
        refused(-1, sources=bad(**change), obstacles=arr)
    pkg.scalars_couple_host(rec, sp, values, sources=bad(shape=pkg.SPH_SOURCE_SPHERE, size=(1.0, 0.0, 0.0)), obstacles=arr)   # a sphere uses size[0] only
    refused(-1, sources=[pkg.scalar_source(**ok)] * 9, obstacles=arr)                                                          # more than SPH_MAX_SCALAR_SOURCES
    refused(-1, beta=(np.nan, 0.0), ref=(0.0, 0.0))
    refused(-1, beta=(1.0, 0.0), ref=(0.0, np.inf))
    refused(-3, sources=[pkg.scalar_source(**ok)], obstacles=arr[:1])                                                          # a dangling body index
    L = pkg.load_library()
    pf = C.POINTER(C.c_float)
    one = np.ones(2, F)
    r2, v2 = rec.copy(), values.copy()
    args = lambda beta, ref, src, n: (r2.ctypes.data, len(r2), C.byref(sp), C.c_float(-1.0), v2.ctypes.data, 2, beta, ref, src, n, None, 0, None, None)
    assert L.sph_scalars_couple_host(*args(one.ctypes.data_as(pf), None, None, 0)) == -1                                       # beta without ref
    assert L.sph_scalars_couple_host(*args(None, None, None, 1)) == -1 and b"null" in L.sph_last_error()                       # a count without data
    assert L.sph_scalars_couple_host(r2.ctypes.data, len(r2), C.byref(sp), C.c_float(-1.0), v2.ctypes.data, 5, None, None, None, 0, None, 0, None, None) == -1
    assert r2.tobytes() == rec.tobytes() and v2.tobytes() == values.tobytes()
    # the defaults and the record's layout
    s = pkg.SphScalarSource()
    L.sph_scalar_source_default(C.byref(s))
    assert (s.shape, s.channel, s.mode, s.body, list(s.center), list(s.size), s.rate, s.target) == (0, 0, 0, -1, [0, 0, 0], [1, 1, 1], 0, 0)
    assert pkg.SPH_MAX_SCALAR_SOURCES == 8 and (pkg.SPH_SOURCE_RATE, pkg.SPH_SOURCE_RELAX, pkg.SPH_SOURCE_SPHERE, pkg.SPH_SOURCE_BOX) == (0, 1, 0, 1)


def test_record_layout_matches_the_header(pkg, tmp_path):
    size, offsets, extra = support.c_layout("SphScalarSource", pkg.SphScalarSource,
                                            ['printf("%d %d %d %d %d\\n", SPH_MAX_SCALAR_SOURCES, SPH_SOURCE_SPHERE, SPH_SOURCE_BOX, SPH_SOURCE_RATE, SPH_SOURCE_RELAX);'],
                                            tmp_path)
    assert size == 64 == C.sizeof(pkg.SphScalarSource) == pkg.SOURCE_DTYPE.itemsize
    assert offsets == [(name, getattr(pkg.SphScalarSource, name).offset) for name, _ in pkg.SphScalarSource._fields_]
    assert extra == ["8 0 1 0 1"]
    assert [pkg.SOURCE_DTYPE.fields[n][1] for n in CR.SOURCE_DTYPE.names] == [CR.SOURCE_DTYPE.fields[n][1] for n in CR.SOURCE_DTYPE.names]


def test_cpp_twin_compiles(pkg):
    support.check_shim_syntax()


# ---- the sign: warm fluid rises --------------------------------------------------------------------
BETA, DC, SUBSTEPS = 4.0, 1.0, 16


def _pool_run(pkg, oracle, rec, sp, values, beta):
    op = to_oracle_params(oracle, sp)
    for _ in range(SUBSTEPS):
        rec = oracle.substep(rec, op, dt=-1.0)
        rec, values, _, _ = pkg.scalars_couple_host(rec, sp, values, beta=beta, ref=0.0)
    return rec


def test_warm_blob_rises_in_the_settled_pool(pkg, oracle):
    """A blob of c = DC in the settled pool, beta = BETA: the free displacement 0.5 beta DC |g| t^2 over SUBSTEPS substeps exceeds one h,
    so the blob's mean height must be strictly higher than in the same run with beta = 0 (no tolerance)."""
    fx = np.load(os.path.join(support.G, "settled_pool.npz"))
    rec, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    t = SUBSTEPS * float(sp.param_timeStep)
    free = 0.5 * BETA * DC * abs(float(sp.param_gravityY)) * t * t
    assert free > float(sp.param_h), (free, sp.param_h)
    fluid = rec["isGhost"] == 0
    c, E = support.fluid_block(rec)
    d = rec["pos"][:, :3] - c
    blob = fluid & ((d * d).sum(axis=1) < (0.3 * E) ** 2)
    assert 100 < blob.sum() < 0.5 * fluid.sum()
    values = np.where(blob, F(DC), F(0)).astype(F)
    warm = _pool_run(pkg, oracle, rec, sp, values, BETA)
    cold = _pool_run(pkg, oracle, rec, sp, values, 0.0)
    assert np.isfinite(warm["pos"][fluid, :3]).all()
    rise = float(warm["pos"][blob, 1].astype(np.float64).mean() - cold["pos"][blob, 1].astype(np.float64).mean())
    print(f"blob of {int(blob.sum())} particles: free displacement {free:.3f}, h {sp.param_h:.3f}, mean height above the beta = 0 run {rise:.4f}")
    assert rise > 0.0
    assert cold[~blob].tobytes() != warm[~blob].tobytes()                    # the surrounding fluid makes way
