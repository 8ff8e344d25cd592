"""Passive tracers on the GPU (include/sph_abi.h "passive tracers").

Every comparison is bitwise and covers every tracer.  Three statements of the same thing are compared: the engine's tracers, the host
loop over the EXISTING interface on a second engine (s = sample(x); dispatch(dt); x = x + dt * s.vel, in numpy fp32), and the numpy
restatement tests/tracer_ref.py on top of the oracle."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT, assert_records_equal, small_scene, to_oracle_params
import tracer_ref as T
from support import build_example, engine, identity_states, run_example

pytestmark = pytest.mark.gpu

F = np.float32
G = os.path.join(ROOT, "tests", "golden")


def _refresh_interval(pkg):
    src = open(os.path.join(ROOT, pkg.__name__, "csrc", "sph_tracer.h")).read()
    return int(re.search(r"#define SPH_TRACER_REFRESH\s+(\d+)", src).group(1))


def _seeds(pkg, rec, sp, rng, n_fluid=160, n_box=160, n_out=40):
    """Fluid particle positions, random points of the grid's box (some dry), points outside the grid, one NaN, one duplicate pair;
    (m, 4) with an initial age."""
    g = pkg.compute_grid_extents(sp)
    lo = np.array(list(g.gridMin), F)
    hi = lo + F(g.cellSize) * np.array(list(g.dims), F)
    fluid = rec["pos"][rec["isGhost"] == 0][:, :3]
    parts = [fluid[rng.choice(len(fluid), min(n_fluid, len(fluid)), replace=False)],
             (lo + (hi - lo) * rng.random((n_box, 3))).astype(F),
             (lo - F(2) + (hi - lo + F(4)) * rng.random((n_out, 3))).astype(F)]
    far = np.array([[hi[0] + 3, lo[1] - 3, 0.5 * (lo[2] + hi[2])], [lo[0] - 50, hi[1] + 50, hi[2] + 50]], F)   # certainly outside the grid
    nan = fluid[:1].copy()
    nan[0, 1] = np.nan
    dup = np.repeat(fluid[7:8], 2, axis=0)
    xyz = np.concatenate(parts + [far, nan, dup]).astype(F)
    p4 = np.zeros((len(xyz), 4), F)
    p4[:, :3] = xyz
    p4[:, 3] = rng.random(len(xyz)).astype(F)
    p4[-1, 3] = p4[-2, 3]                                                # (the duplicate pair: same point, same age)
    return p4, len(xyz) - 3, (len(xyz) - 2, len(xyz) - 1)               # index of the NaN tracer, indices of the duplicate pair


def _host_step(f, tr, dt, integ, dispatch_dt=-1.0):
    """One substep of the host loop on engine f: sample, dispatch, move (numpy fp32: a multiply, then an add)."""
    dt = F(dt)
    x = tr["pos"].copy()
    fin = np.isfinite(x).all(axis=1)
    s = f.sample(x)
    v = s["vel"]
    with np.errstate(all="ignore"):
        if integ == T.MIDPOINT:
            xm = (x + (F(F(0.5) * dt) * v).astype(F)).astype(F)
            v = f.sample(xm)["vel"]
        f.DispatchCompute(dispatch_dt)
        moved = (x + (dt * v).astype(F)).astype(F)
    out = tr.copy()
    out["pos"] = np.where(fin[:, None], moved, x)                       # a non-finite tracer keeps its position bits
    out["vel"] = np.where(fin[:, None], v, F(0))
    out["fraction"] = np.where(fin, s["fraction"], F(0))
    out["age"] = (tr["age"] + dt).astype(F)
    return out


def _host_loop(f, p4, n, dt, integ, dispatch_dt=-1.0, snapshots=None):
    tr = T.seed(p4)
    if snapshots is not None:
        snapshots.append(T.snapshot_of(tr))
    for _ in range(n):
        tr = _host_step(f, tr, dt, integ, dispatch_dt)
        if snapshots is not None:
            snapshots.append(T.snapshot_of(tr))
    return tr


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    for name in ("pos", "vel", "fraction", "age"):
        x, y = np.ascontiguousarray(a[name]).view(np.uint32), np.ascontiguousarray(b[name]).view(np.uint32)
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(len(a), -1).any(axis=1))[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)}/{len(a)} tracers; first i={i}: {a[name][i]!r} vs {b[name][i]!r}")


def test_tracers_equal_the_host_loop_and_the_reference(pkg, oracle):
    n = 10
    for name, rec, sp in identity_states(pkg):
        op = to_oracle_params(oracle, sp)
        p4, i_nan, (d0, d1) = _seeds(pkg, rec, sp, np.random.default_rng(17))
        dt = F(sp.param_timeStep)
        for integ in (T.EULER, T.MIDPOINT):
            want, want_rec = T.run(oracle, rec, op, p4, n, integ)
            assert (want["pos"][:160] != p4[:160, :3]).any(axis=1).sum() > (80 if rec["density"].any() else 0), name
            assert (want["fraction"] == 0).sum() > 20 and (want["fraction"] > 0.5).sum() > 60, name
            for kern in (1, 2, 3):
                for aos in (0, 1):
                    what = f"{name} integrator {integ} pass {kern} aos {aos}"
                    f = engine(pkg, rec, sp, kern, aos)
                    f.set_tracers(p4, integ)
                    assert f.num_tracers() == len(p4)
                    for _ in range(n):
                        f.DispatchCompute()
                    got, got_rec = f.tracers(), f.download()
                    assert f.tracer_info()[0] == n
                    f.close()
                    h = engine(pkg, rec, sp, kern, aos)
                    loop = _host_loop(h, p4, n, dt, integ)
                    loop_rec = h.download()
                    h.close()
                    p = engine(pkg, rec, sp, kern, aos)                  # no tracers, no sampling
                    for _ in range(n):
                        p.DispatchCompute()
                    plain_rec = p.download()
                    p.close()
                    _same(got, loop, what + " (host loop)")
                    _same(got, want, what + " (tracer_ref)")
                    assert_records_equal(got_rec, plain_rec, what + ": records with and without tracers")
                    assert_records_equal(got_rec, loop_rec, what + ": records of the host loop's engine")
                    assert_records_equal(got_rec, want_rec, what + ": records of the oracle")
                    assert np.array_equal(got["pos"][i_nan].view(np.uint32), p4[i_nan, :3].view(np.uint32)) and not got["vel"][i_nan].any()
                    assert got[d0].tobytes() == got[d1].tobytes()


def test_first_substep_on_records_without_a_density_moves_nothing(pkg):
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    assert not rec["density"].any()
    rec = rec.copy()
    rec["vel"][:, :3] = F(1.5)
    p4 = np.zeros((256, 4), F)
    p4[:, :3] = rec["pos"][::16, :3]
    f = engine(pkg, rec, sp)
    f.set_tracers(p4, T.MIDPOINT)
    f.DispatchCompute()
    a = f.tracers()
    assert np.array_equal(a["pos"].view(np.uint32), p4[:, :3].view(np.uint32)) and not a["vel"].any() and not a["fraction"].any()
    assert np.all(a["age"] == F(sp.param_timeStep))
    f.DispatchCompute()
    b = f.tracers()
    f.close()
    assert (b["pos"] != p4[:, :3]).any(axis=1).all() and np.all(b["fraction"] > 0)


def test_graph_replay_equals_eager_dispatch(pkg):
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    p4, _, _ = _seeds(pkg, rec, sp, np.random.default_rng(23))
    for integ in (T.EULER, T.MIDPOINT):
        for aos in (0, 1):
            g = engine(pkg, rec, sp, 3, aos, graph=1)
            e = engine(pkg, rec, sp, 3, aos, graph=0)
            for f in (g, e):
                f.set_tracers(p4, integ, history=4, stride=3)
            for _ in range(5):
                g.DispatchN(4)
                for _ in range(4):
                    e.DispatchCompute()
            launches = g.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
            assert launches >= 3, launches
            what = f"graph, integrator {integ}, aos {aos}"
            _same(g.tracers(), e.tracers(), what)
            assert g.tracer_info() == e.tracer_info() == (20, 4, 3)
            (gf, gh), (ef, eh) = g.tracer_history(), e.tracer_history()
            assert gf == ef == 3 and gh.tobytes() == eh.tobytes(), what
            assert_records_equal(g.download(), e.download(), what)
            # without tracers (a graph captured WITH them must not serve this call), and back
            before = g.tracers()
            for f in (g, e):
                f.clear_tracers()
            for _ in range(3):
                g.DispatchN(4)
                for _ in range(4):
                    e.DispatchCompute()
            assert g.num_tracers() == 0 and len(g.tracers()) == 0
            assert_records_equal(g.download(), e.download(), what + ", tracers dropped")
            for f in (g, e):
                f.set_tracers(before["pos"], integ, history=4, stride=3)
            for _ in range(3):
                g.DispatchN(4)
                for _ in range(4):
                    e.DispatchCompute()
            assert g.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) > launches
            _same(g.tracers(), e.tracers(), what + ", tracers set again")
            assert g.tracer_info() == e.tracer_info() == (12, 4, 1)
            assert g.tracer_history()[1].tobytes() == e.tracer_history()[1].tobytes(), what
            assert_records_equal(g.download(), e.download(), what + ", tracers set again")
            g.close()
            e.close()


def test_history_ring(pkg):
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    p4, _, _ = _seeds(pkg, rec, sp, np.random.default_rng(29))
    n = 8
    step = engine(pkg, rec, sp)                                          # the stepwise run: a download after every substep
    step.set_tracers(p4, T.MIDPOINT)
    snaps = [T.snapshot_of(step.tracers())]
    for _ in range(n):
        step.DispatchCompute()
        snaps.append(T.snapshot_of(step.tracers()))
    step.close()
    assert snaps[0].tobytes() == p4.tobytes()                            # snapshot 0 is the seed
    for K, S in ((3, 1), (2, 3), (16, 1), (1, 1), (5, 3)):
        f = engine(pkg, rec, sp)
        f.set_tracers(p4, T.MIDPOINT, history=K, stride=S)
        first, hist = f.tracer_history()
        assert first == 0 and hist.shape == (1, len(p4), 4) and hist[0].tobytes() == p4.tobytes()
        for c in range(1, n + 1):
            f.DispatchCompute()
            if c in (1, 4, n):
                count, want_first = T.history_stored(c, S, K)
                first, hist = f.tracer_history()
                assert (first, len(hist)) == (want_first, count) and f.tracer_info() == (c, count, want_first), (K, S, c)
                for j in range(count):
                    assert hist[j].tobytes() == snaps[(first + j) * S].tobytes(), (K, S, c, j)
        f.close()
    assert T.history_stored(n, 1, 3) == (3, 6)                           # (K smaller than the number of snapshots: the ring wrapped)


def test_order_independence_across_a_refresh_of_the_processing_order(pkg):
    R = _refresh_interval(pkg)
    n = R + 9
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    rng = np.random.default_rng(31)
    p4, _, (d0, d1) = _seeds(pkg, rec, sp, rng, 600, 300, 60)
    perm = rng.permutation(len(p4))
    for integ in (T.EULER, T.MIDPOINT):
        a = engine(pkg, rec, sp)
        a.set_tracers(p4, integ, history=3, stride=R // 2)
        b = engine(pkg, rec, sp)
        b.set_tracers(p4[perm], integ, history=3, stride=R // 2)
        a.DispatchN(n)                                                   # one call ...
        for _ in range(n):                                               # ... and single dispatches
            b.DispatchCompute()
        ta, tb = a.tracers(), b.tracers()
        (fa, ha), (fb, hb) = a.tracer_history(), b.tracer_history()
        assert_records_equal(a.download(), b.download(), "permuted seeds")
        a.close()
        b.close()
        _same(ta[perm], tb, f"permuted seeds, integrator {integ}")
        assert fa == fb and ha[:, perm].tobytes() == hb.tobytes()
        assert ta[d0].tobytes() == ta[d1].tobytes()
        h = engine(pkg, rec, sp)                                         # the host loop has no processing order at all
        loop = _host_loop(h, p4, n, F(sp.param_timeStep), integ)
        h.close()
        _same(ta, loop, f"{n} substeps against the host loop, integrator {integ}")


def test_fountain_river_pause_and_override_dt(pkg, oracle):
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    p4, _, _ = _seeds(pkg, rec, sp, np.random.default_rng(37))
    dt = F(sp.param_timeStep)
    # fountain mode: tracers see the entry state, before the recycle of the same dispatch
    pair = [engine(pkg, rec, sp), engine(pkg, rec, sp)]
    for f in pair:
        f.fountainMode = 1
        f.fountainOffset = (0.0, -1.0, 0.0)
        f.fountainDrainPerSec = 200.0
        f.fountainDrainLevel = 1.5
    pair[0].set_tracers(p4, T.MIDPOINT)
    for _ in range(6):
        pair[0].DispatchCompute()
    loop = _host_loop(pair[1], p4, 6, dt, T.MIDPOINT)
    _same(pair[0].tracers(), loop, "fountain mode")
    assert_records_equal(pair[0].download(), pair[1].download(), "fountain mode")
    assert pair[0].fountainSeed == 6
    for f in pair:
        f.close()
    # river mode
    import test_gpu_river
    P, rsp, _, river, _, heights = test_gpu_river._scene(pkg, oracle)
    P = oracle.substep_river(P, to_oracle_params(oracle, rsp), oracle.ORiver.from_buffer_copy(bytes(river)), heights, steps=2)   # densities
    r4, _, _ = _seeds(pkg, P, rsp, np.random.default_rng(41))
    pair = [engine(pkg, P, rsp), engine(pkg, P, rsp)]
    for f in pair:
        f.set_river(river, heights)
    pair[0].set_tracers(r4, T.EULER)
    for _ in range(6):
        pair[0].DispatchCompute()
    loop = _host_loop(pair[1], r4, 6, F(rsp.param_timeStep), T.EULER)
    got = pair[0].tracers()
    _same(got, loop, "river mode")
    assert (got["pos"] != r4[:, :3]).any(axis=1).sum() > 100
    assert_records_equal(pair[0].download(), pair[1].download(), "river mode")
    for f in pair:
        f.close()
    # param_pause: no substep, no move, no ageing, c unchanged
    f = engine(pkg, rec, sp)
    f.set_tracers(p4, T.MIDPOINT, history=4)
    f.DispatchN(3)
    a = f.tracers()
    f.param_pause = 1
    f.DispatchCompute()
    f.DispatchN(4)
    assert f.tracers().tobytes() == a.tobytes() and f.tracer_info() == (3, 4, 0)
    f.param_pause = 0
    f.DispatchCompute()
    assert f.tracer_info()[0] == 4 and np.all(f.tracers()["age"] > a["age"])
    f.close()
    # overrideDt: the step and the age use it
    odt = F(0.6) * dt
    f, h = engine(pkg, rec, sp), engine(pkg, rec, sp)
    f.set_tracers(p4, T.MIDPOINT)
    for _ in range(5):
        f.DispatchCompute(float(odt))
    loop = _host_loop(h, p4, 5, odt, T.MIDPOINT, dispatch_dt=float(odt))
    got = f.tracers()
    _same(got, loop, "overrideDt")
    want_age = p4[:, 3].copy()
    for _ in range(5):
        want_age = (want_age + odt).astype(F)
    assert np.array_equal(got["age"], want_age)
    assert_records_equal(f.download(), h.download(), "overrideDt")
    ref, _ = T.run(oracle, rec, to_oracle_params(oracle, sp), p4, 5, T.MIDPOINT, dt=float(odt))
    _same(got, ref, "overrideDt (tracer_ref)")
    f.close()
    h.close()


def test_refusals_and_lifetimes(pkg):
    import torch
    L = pkg.load_library()
    vp = C.c_void_p
    rec = np.load(os.path.join(G, "scene4096.npz"))["after_10"]
    _, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    p4, _, _ = _seeds(pkg, rec, sp, np.random.default_rng(43))
    m = len(p4)
    ptr = p4.ctypes.data_as(vp)
    # a z-slab engine
    from importlib import import_module
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    assert L.sph_tracers_set(slab._h, ptr, m, 1, 0, 1) == -3 and b"slab" in L.sph_last_error()
    assert L.sph_tracers_count(slab._h) == 0
    slab.close()
    f = engine(pkg, rec, sp)
    h = f._h
    # SPH_OPT_GRID_BUILD 1: at set ...
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.set_tracers(p4)
    assert f.num_tracers() == 0
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    f.set_tracers(p4, T.EULER, history=2)
    f.DispatchCompute()
    a, rec_a = f.tracers(), f.download()
    # ... and at dispatch: refused, nothing moves
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.DispatchCompute()
    with pytest.raises(pkg.SphError, match="-3"):
        f.DispatchN(3)
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
    assert f.tracers().tobytes() == a.tobytes() and f.tracer_info() == (1, 2, 0)
    assert_records_equal(f.download(), rec_a, "after the refused dispatches")
    # bad arguments
    dev = torch.zeros(4 * m, dtype=torch.float32, device="cuda")
    assert L.sph_tracers_set(h, None, m, 1, 0, 1) == -1
    assert L.sph_tracers_set_device(h, None, m, 1, 0, 1) == -1
    assert L.sph_tracers_set(None, ptr, m, 1, 0, 1) == -1
    assert L.sph_tracers_set(h, ptr, m, 2, 0, 1) == -1 and L.sph_tracers_set(h, ptr, m, -1, 0, 1) == -1
    assert L.sph_tracers_set(h, ptr, m, 1, 4, 0) == -1
    assert L.sph_tracers_set(h, ptr, m, 1, (2 ** 31 - 1) // m + 1, 1) == -1
    assert L.sph_tracers_set_device(h, vp(dev.data_ptr()), m, 1, 0xFFFFFFFF, 1) == -1
    assert f.tracers().tobytes() == a.tobytes() and f.tracer_info() == (1, 2, 0)      # the refused calls changed nothing
    out = np.zeros(m, pkg.TRACER_DTYPE)
    assert L.sph_tracers_download(h, out.ctypes.data_as(vp), m - 1) == -4 and not out.tobytes().strip(b"\0")
    assert L.sph_tracers_download(h, None, m) == -1
    hist = np.zeros((2, m, 4), F)
    assert L.sph_tracers_history(h, hist.ctypes.data_as(vp), 1, None, None) == -4 and not hist.any()
    assert L.sph_tracers_history(h, hist.ctypes.data_as(vp), 2, None, None) == 0 and hist[0].tobytes() == p4.tobytes()
    assert f.tracers_device() != 0
    # the device variants: set from a device array, read through the borrowed pointer
    dev.copy_(torch.from_numpy(p4.reshape(-1)))
    f.set_tracers_device(dev.data_ptr(), m, T.EULER, history=2)
    f.DispatchCompute()
    f.sync()
    got = f.tracers()
    view = np.zeros(m, pkg.TRACER_DTYPE)
    hip = C.CDLL("libamdhip64.so.7")                                      # (already loaded by the engine)
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(view.ctypes.data_as(vp), vp(f.tracers_device()), 32 * m, 2) == 0          # hipMemcpyDeviceToHost
    assert view.tobytes() == got.tobytes()
    g2 = engine(pkg, rec, sp)                                            # the host variant on a fresh engine with the same history of calls
    g2.DispatchCompute()
    g2.set_tracers(p4, T.EULER, history=2)
    g2.DispatchCompute()
    assert got.tobytes() == g2.tracers().tobytes() and f.tracer_history()[1].tobytes() == g2.tracer_history()[1].tobytes()
    g2.close()
    # history without a ring, M = 0
    f.set_tracers(p4, T.EULER, history=0)
    with pytest.raises(pkg.SphError, match="-3"):
        f.tracer_history()
    assert f.tracer_info() == (0, 0, 0)
    f.clear_tracers()
    assert f.num_tracers() == 0 and len(f.tracers()) == 0 and f.tracers_device() == 0 and f.tracer_info() == (0, 0, 0)
    with pytest.raises(pkg.SphError, match="-3"):
        f.tracer_history()
    f.set_tracers(np.zeros((0, 3), F))
    f.DispatchCompute()
    assert f.num_tracers() == 0
    # sph_tracers_set twice: the second set replaces the first and restarts c and the history
    f.set_tracers(p4, T.MIDPOINT, history=3)
    f.DispatchN(5)
    assert f.tracer_info() == (5, 3, 3)
    q4 = p4[: m // 2].copy()
    f.set_tracers(q4, T.EULER, history=3)
    assert f.num_tracers() == len(q4) and f.tracer_info() == (0, 1, 0)
    first, hist = f.tracer_history()
    assert first == 0 and hist.shape == (1, len(q4), 4) and hist[0].tobytes() == q4.tobytes()
    t = f.tracers()
    assert t["pos"].tobytes() == q4[:, :3].tobytes() and np.array_equal(t["age"], q4[:, 3]) and not t["vel"].any() and not t["fraction"].any()
    f.DispatchCompute()
    assert f.tracer_info() == (1, 2, 0)
    # sph_reset drops the set
    f.ResetSimulation()
    assert f.num_tracers() == 0 and f.tracer_info() == (0, 0, 0)
    f.DispatchCompute()
    f.close()
    # N = 0 particles: nothing to carry the tracers
    z = engine(pkg, rec[:0], sp)
    z.set_tracers(p4, T.MIDPOINT, history=2)
    z.DispatchN(3)
    t = z.tracers()
    fin = np.isfinite(p4[:, :3]).all(axis=1)
    assert np.array_equal(t["pos"][fin], p4[fin, :3]) and not t["vel"].any() and not t["fraction"].any()
    assert np.array_equal(t["pos"].view(np.uint32)[~fin], p4[~fin, :3].view(np.uint32))
    assert z.tracer_info() == (3, 2, 2)
    z.close()


def test_full_size_against_the_host_loop(pkg):
    """BASELINE.json configs[2] (4 194 304 particles, 128^3 cells) with 1 048 576 tracers, 3 substeps, both integrators."""
    syn = pkg.synthetic
    cfg = syn.CONFIGS[3]
    rec, _ = syn.make_particles(cfg)
    sp = pkg.default_params(**syn.params_fields(cfg))
    rng = np.random.default_rng(47)
    lo, hi = rec["pos"][:, :3].min(axis=0), rec["pos"][:, :3].max(axis=0)
    m = 1 << 20
    p4 = np.zeros((m, 4), F)
    p4[:, :3] = (lo - F(0.3) + (hi - lo + F(0.6)) * rng.random((m, 3))).astype(F)
    p4[5, 0] = np.nan
    for integ in (T.MIDPOINT, T.EULER):
        f = pkg.SPHFluidGPU.from_particles(rec, sp)
        f.DispatchCompute()                                              # (the spawned records carry no density yet)
        h = pkg.SPHFluidGPU.from_particles(rec, sp)
        h.DispatchCompute()
        f.set_tracers(p4, integ, history=2, stride=3)
        f.DispatchN(3)
        got = f.tracers()
        first, hist = f.tracer_history()
        loop = _host_loop(h, p4, 3, F(sp.param_timeStep), integ)
        _same(got, loop, f"configs[2], integrator {integ}")
        assert first == 0 and hist[0].tobytes() == p4.tobytes() and hist[1].tobytes() == T.snapshot_of(got).tobytes()
        moved = (got["pos"] != p4[:, :3]).any(axis=1).sum()
        print(f"configs[2], integrator {integ}: {moved} of {m} tracers moved, {(got['fraction'] >= 0.5).sum()} in the fluid")
        assert moved > m // 2
        if integ == T.EULER:
            assert_records_equal(f.download(), h.download(), "configs[2]: records with tracers and of the host loop's engine")
        f.close()
        h.close()


def _parse_pathlines(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    ne = int(re.search(rb"element edge (\d+)", head).group(1))
    v = np.frombuffer(body[: 16 * nv], "<f4").reshape(nv, 4)
    e = np.frombuffer(body[16 * nv: 16 * nv + 8 * ne], "<i4").reshape(ne, 2)
    assert len(body) == 16 * nv + 8 * ne
    return v, e


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pathlines_example(pkg, tmp_path):
    ply = tmp_path / "pathlines.ply"
    frames = 4
    res = run_example(build_example(pkg, "pathlines", tmp_path), [ply, frames], timeout=300)
    assert res.returncode == 0 and "pathlines OK" in res.stdout
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("frame ")]
    assert len(lines) == frames
    # the same run through the Python mirror
    i = np.arange(32, dtype=F)
    p4 = np.zeros((32, 32, 4), F)
    p4[:, :, 0] = (F(-5.5) + F(9.0) * i / F(31.0))[None, :]
    p4[:, :, 1] = F(-4.0)
    p4[:, :, 2] = (F(-5.5) + F(10.5) * i / F(31.0))[:, None]
    p4 = p4.reshape(-1, 4)
    f = pkg.SPHFluidGPU(50000, seed=7)
    f.set_tracers(p4, pkg.SPH_TRACER_MIDPOINT, history=frames + 1, stride=16)
    phase = F(0.0)
    for k, ln in enumerate(lines):
        f.ApplyWaveImpulse(1.5, 3.0, float(phase), (0.0, 1.0, 0.0))
        phase = F(phase + F(4.0) / F(60.0))
        f.DispatchN(16, float(f.param_timeStep))
        t = f.tracers()
        count = int(ln.split("in_fluid=")[1].split()[0])
        assert count == int((t["fraction"] >= 0.5).sum()), (k, ln)
        assert abs(float(ln.split("mean_age=")[1]) - float(t["age"].astype(np.float64).mean())) < 1e-5
    assert int(lines[-1].split("in_fluid=")[1].split()[0]) > 500
    first, hist = f.tracer_history()
    f.close()
    v, e = _parse_pathlines(ply)
    assert first == 0 and v.tobytes() == hist.tobytes()
    assert len(e) == frames * 1024 and np.array_equal(e[:, 1] - e[:, 0], np.full(len(e), 1024))
    mine = tmp_path / "mine.ply"
    pkg.write_pathlines_ply(str(mine), hist)
    v2, e2 = _parse_pathlines(mine)
    assert v2.tobytes() == v.tobytes() and np.array_equal(e2, e)
