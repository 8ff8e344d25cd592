"""Secondary particles without a GPU: the library exports the interface, sph_diffuse_step_host equals the numpy restatement
(tests/diffuse_ref.py) bit for bit, and the restatement against facts that follow from DESIGN.md section 3j.

The shared scene (diffuse_ref.scene) is run for 24 substeps by the oracle, the numpy sampler and the rule; the run itself must contain
every event the GPU tests compare, so that none of them can pass vacuously.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import diffuse_ref as D

F = np.float32
DIFFUSE_SYMBOLS = ("sph_diffuse_default", "sph_diffuse_set", "sph_diffuse_get", "sph_diffuse_info", "sph_diffuse_download",
                   "sph_diffuse_device", "sph_diffuse_seed", "sph_diffuse_step_host")


def test_library_exports_the_diffuse_interface(pkg):
    L = pkg.load_library()
    for name in DIFFUSE_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphDiffuse) == 48 and C.sizeof(pkg.SphDiffuseConfig) == 64 and C.sizeof(pkg.SphDiffuseInfo) == 88
    assert pkg.DIFFUSE_DTYPE == D.DIFFUSE_DTYPE
    assert [pkg.DIFFUSE_DTYPE.fields[f][1] for f in ("pos", "life", "vel", "age", "parent", "birth", "kind", "pad")] == [0, 12, 16, 28, 32, 36, 40, 44]
    assert (pkg.SPH_DIFFUSE_SPRAY, pkg.SPH_DIFFUSE_FOAM, pkg.SPH_DIFFUSE_BUBBLE) == (0, 1, 2) == (D.SPRAY, D.FOAM, D.BUBBLE)
    src = open(os.path.join(ROOT, "include", "sph_abi.h")).read()
    assert ("typedef struct SphDiffuse { float pos[3]; float life; float vel[3]; float age; uint32_t parent; uint32_t birth; uint32_t kind; "
            "uint32_t pad; } SphDiffuse;") in src
    assert "#define SPH_ABI_VERSION 4 " in src
    eng = open(os.path.join(ROOT, pkg.__name__, "csrc", "sph_engine.hip")).read()
    assert "static_assert(sizeof(SphDiffuse) == 48" in eng                # the C side of the same fact, checked when the library is built
    for m in ("set_diffuse", "diffuse", "diffuse_device", "diffuse_info", "seed_diffuse", "clear_diffuse"):
        assert hasattr(pkg.SPHFluidGPU, m), m
    for f in ("diffuse_config", "diffuse_step_host", "write_points_ply"):
        assert callable(getattr(pkg, f)), f
    cfg = pkg.diffuse_config()
    assert cfg.capacity == 65536 and 1 <= cfg.maxPerParent <= 8 and cfg.sprayBelow <= cfg.bubbleAbove and 0.0 <= cfg.kd <= 1.0
    assert pkg.diffuse_config(capacity=7, kd=0.25).capacity == 7


# hash(seed, id, counter, draw) of DESIGN.md section 3j, worked out when the section was written
KNOWN = (((0, 0, 0, 0), 0x0eaa7511), ((1, 2, 3, 4), 0x2d47a7e5), ((11, 4095, 23, 0), 0x8929a1fa),
         ((0xFFFFFFFF, 0xFFFFFFFF, (1 << 40) + 5, 33), 0xc9be4936))


def test_hash_known_answers(pkg):
    assert [int(x) for x in D.mix(np.array([0, 1, 2, 0xFFFFFFFF]))] == [0x0, 0x688990c0, 0xd1132181, 0x6768824a]
    for (seed, pid, c, draw), want in KNOWN:
        assert int(D.hash32(seed, np.array([pid]), c, np.array([draw]))[0]) == want
        u = D.uniform(seed, np.array([pid]), c, np.array([draw]))[0]
        assert u == F((want >> 8) * 2.0 ** -24) and 0.0 <= u < 1.0
    # the library's hash through the one place it shows unscaled: life = 0 + U_4 (1 - 0) of child 0 of particle 2 at counter 3, seed 1
    sp = pkg.default_params()
    rec = np.zeros(3, pkg.PARTICLE_DTYPE)
    rec["density"], rec["padA"] = 1000.0, [0.0, 0.0, 1.0]
    cfg = pkg.diffuse_config(capacity=8, seed=1, threshold=0.0, rate=1.0 / sp.param_timeStep, lifeMin=0.0, lifeMax=1.0, maxPerParent=1)
    out, info = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 3)
    assert len(out) == 1 and info["spawned"] == 1 and out["parent"][0] == 2 and out["birth"][0] == 3 and out["kind"][0] == D.FOAM
    assert out["life"][0] == F((0x2d47a7e5 >> 8) * 2.0 ** -24)


def _samples(pkg, u, n):
    s = np.zeros(len(n), pkg.SAMPLE_DTYPE)
    s["vel"], s["count"] = u, n
    return s


@pytest.mark.parametrize("capacity", [None, 64])
def test_host_step_equals_the_restatement_over_the_scene(pkg, oracle, capacity):
    rec, sp, op, pool = D.scene(pkg, oracle)
    cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, **({} if capacity is None else {"capacity": capacity})))
    want = D.scene_reference(pkg, oracle, capacity)
    totals = {"seeded": len(pool), "alive": len(pool)}
    for i in range(D.SCENE_STEPS):
        b = oracle.build_grid(rec, op)
        u, n = D.sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
        pool, totals = pkg.diffuse_step_host(cfg, sp, pool, _samples(pkg, u, n), rec, i, totals=totals)
        rec = oracle.substep(rec, op)
        ref_pool, ref_t = want[i]
        assert pool.tobytes() == ref_pool.tobytes(), i
        assert {k: totals[k] for k in ref_t} == ref_t, i
        assert totals["alive"] == totals["seeded"] + totals["spawned"] - totals["dropped"] - sum(totals[k] for k in ("diedLife", "diedAge", "leftBox", "nonFinite"))


def test_the_scene_contains_every_event(pkg, oracle):
    snaps = D.scene_reference(pkg, oracle)
    pools, totals = [s[0] for s in snaps], [s[1] for s in snaps]
    last = totals[-1]
    kinds = np.concatenate([p["kind"][p["age"] > 0] for p in pools])          # classes given by a substep, not the newborn's label
    assert all((kinds == q).sum() > 0 for q in (D.SPRAY, D.FOAM, D.BUBBLE))
    assert last["diedLife"] > 0 and last["leftBox"] > 0 and last["diedAge"] > 0 and last["nonFinite"] == 1
    p = pools[0]
    newborn = p[p["age"] == 0]
    assert np.bincount(newborn["parent"]).max() > 1                          # a spawn with more than one child
    alive = [len(D.scene(pkg, oracle)[3])] + [t["alive"] for t in totals]       # from the four seeded records on
    assert min(alive) < 64 < max(alive) and min(alive) < 256 < max(alive)    # the count crosses a wave and a block boundary
    small = D.scene_reference(pkg, oracle, 64)
    assert small[-1][1]["dropped"] > 0 and max(t["alive"] for _, t in small) == 64
    assert last["dropped"] > 0 and max(alive) <= 4096                        # (and the large pool fills up too, late in the run)


def test_stable_compaction_and_overflow_order(pkg, oracle):
    rec, sp, op, _ = D.scene(pkg, oracle)
    b = oracle.build_grid(rec, op)
    pool = np.zeros(40, D.DIFFUSE_DTYPE)
    pool["pos"] = rec["pos"][100:140, :3]
    pool["life"] = np.where(np.arange(40) % 3 == 0, 0.0, 1.0)               # every third record dies, whatever its class (life' <= 0)
    pool["parent"] = np.arange(40) + 1000                                    # a label that travels with the record
    cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, capacity=60, maxAge=10.0))
    u, n = D.sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
    for out, t in (D.step(pool, u, n, rec, cfg, op.h, tuple(op.gravity), b["grid"], F(op.timeStep), 5),
                   pkg.diffuse_step_host(cfg, sp, pool, _samples(pkg, u, n), rec, 5)):
        keep = [i + 1000 for i in range(40) if i % 3]
        assert list(out["parent"][:len(keep)]) == keep                       # the survivors, in their order
        born = out[len(keep):]
        assert len(out) == 60 and len(born) == 60 - len(keep) and t["dropped"] == t["spawned"] - len(born) > 0
        cnt = D.children(rec, cfg, F(op.timeStep), 5)
        full = np.repeat(np.arange(len(rec)), cnt)                           # (parent ascending, k ascending): the first `room` of them are kept
        assert list(born["parent"]) == list(full[:len(born)])
        assert np.all(born["age"] == 0) and np.all(born["birth"] == 5) and np.all(born["life"] >= F(cfg.lifeMin)) and np.all(born["life"] <= F(cfg.lifeMax))
        off = np.abs(born["pos"].astype(np.float64) - rec["pos"][born["parent"], :3]).max()
        assert off <= cfg.spread * op.h * (1 + 2.0 ** -22)
        assert born["vel"].tobytes() == np.ascontiguousarray(rec["vel"][born["parent"], :3]).tobytes()


def test_who_spawns(pkg, oracle):
    rec, sp, op, _ = D.scene(pkg, oracle)
    rec = rec[:64].copy()
    rec["padA"], rec["density"] = 1.0, 1000.0
    rec["isGhost"][0:8] = 1
    rec["isGhost"][8:12] = 2
    rec["density"][12:16] = 0.0
    rec["density"][16:18] = -1.0
    rec["padA"][18:20] = np.nan
    rec["padA"][20:22] = np.inf
    rec["padA"][22:24] = 0.2                                                 # not ABOVE the threshold
    rec["isActive"][24:32] = 1                                               # isActive says nothing about fluid
    cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, threshold=0.2, maxPerParent=8, rate=1e9))
    cnt = D.children(rec, cfg, F(op.timeStep), 0)
    assert not cnt[:24].any() and np.all(cnt[24:] == 8)
    out, t = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 0)
    assert t["spawned"] == 8 * 40 and sorted(set(out["parent"])) == list(range(24, 64))
    paused = type(sp).from_buffer_copy(sp)
    paused.param_pause = 1
    same, _ = pkg.diffuse_step_host(cfg, paused, out, np.zeros(len(out), pkg.SAMPLE_DTYPE), rec, 1)
    assert same.tobytes() == out.tobytes()                                   # param_pause: nothing happens


BAD = (dict(rate=np.nan), dict(rate=-1.0), dict(lifeMin=np.inf), dict(lifeMin=-0.1), dict(lifeMax=np.nan), dict(spread=-1.0), dict(spread=np.inf),
       dict(lifeMin=0.5, lifeMax=0.25), dict(maxPerParent=0), dict(maxPerParent=9), dict(sprayBelow=7, bubbleAbove=6), dict(kd=-0.01),
       dict(kd=1.01), dict(kd=np.nan), dict(capacity=2 ** 31))


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(d))
def test_config_refusals(pkg, bad):
    cfg = pkg.diffuse_config(**bad)
    with pytest.raises(pkg.SphError, match="diffuse"):
        pkg.diffuse_step_host(cfg, pkg.default_params(), D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), np.zeros(0, pkg.PARTICLE_DTYPE), 0)


def test_points_ply(pkg, tmp_path):
    rec = np.zeros(3, pkg.DIFFUSE_DTYPE)
    rec["pos"] = [(1, 2, 3), (4, 5, 6), (7, 8, 9)]
    rec["kind"] = [0, 1, 2]
    path = tmp_path / "points.ply"
    pkg.write_points_ply(path, rec)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    assert b"element vertex 3" in head and b"property uchar kind" in head and len(body) == 3 * 13
    got = np.frombuffer(body, np.dtype([("pos", "<f4", (3,)), ("kind", "u1")]))
    assert np.array_equal(got["pos"], rec["pos"]) and list(got["kind"]) == [0, 1, 2]
