"""Crest births of the diffuse pool without a GPU: the library exports the interface, sph_diffuse_step_host_crest equals the numpy
restatement (tests/diffuse_crest_ref.py, on shell_host rows) bit for bit, the term off is sph_diffuse_step_host, the foam term's
children stay what they were, births come from where a block's surface is convex and moves outward, and known answers for draw 33 and
for the two clamp windows.

The shared scene (diffuse_ref.scene with diffuse_crest_ref.SCENE_CREST) must itself contain every event the GPU tests compare.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import diffuse_crest_ref as K
import diffuse_ref as D
import shell_scenes

F = np.float32
CREST_SYMBOLS = ("sph_diffuse_crest_default", "sph_diffuse_set_crest", "sph_diffuse_get_crest", "sph_diffuse_crest_info",
                 "sph_diffuse_step_host_crest")


def test_library_exports_the_crest_interface(pkg):
    L = pkg.load_library()
    for name in CREST_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphDiffuseCrest) == 48 and C.sizeof(pkg.SphDiffuseCrestInfo) == 32 and C.sizeof(pkg.SphDiffuseConfig) == 64
    src = open(os.path.join(ROOT, "include", "sph_abi.h")).read()
    assert "#define SPH_ABI_VERSION 4 " in src and "} SphDiffuseCrest;" in src and "} SphDiffuseCrestInfo;" in src
    for m in ("set_diffuse_crest", "clear_diffuse_crest", "diffuse_crest", "diffuse_crest_info"):
        assert hasattr(pkg.SPHFluidGPU, m), m
    c = pkg.diffuse_crest_config()
    assert c.rate > 0 and c.radius <= 0 and c.crestMin < c.crestMax and c.speedMin < c.speedMax and c.align == F(0.6) and c.every == 1
    assert c.offset == F(0.10) and c.minCount == 0 and c.flags == 0
    assert pkg.diffuse_crest_config(every=4, align=0.25).every == 4
    with pytest.raises(pkg.SphError):
        pkg.diffuse_crest_config(nothing=1)


def _samples(pkg, u, n):
    s = np.zeros(len(n), pkg.SAMPLE_DTYPE)
    s["vel"], s["count"] = u, n
    return s


@pytest.mark.parametrize("capacity,every,n", [(K.ROOMY, 1, None), (64, 1, None), (K.ROOMY, 3, None), (K.ROOMY, 1, 4001)])
def test_host_twin_equals_the_restatement_over_the_scene(pkg, oracle, capacity, every, n):
    rec, sp, op, pool = D.scene(pkg, oracle)
    rec = rec if n is None else rec[:n].copy()
    cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, **({} if capacity is None else {"capacity": capacity})))
    crest = K.scene_crest(pkg, sp, every=every)
    want = K.scene_reference(pkg, oracle, capacity, every, n)
    totals = {"seeded": len(pool), "alive": len(pool)}
    for i in range(D.SCENE_STEPS):
        b = oracle.build_grid(rec, op)
        u, cnt = D.sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
        rows = K.shell_rows(pkg, rec, sp, crest)
        pool, totals = pkg.diffuse_step_host(cfg, sp, pool, _samples(pkg, u, cnt), rec, i, totals=totals, crest=crest, shell_rows=rows)
        rec = oracle.substep(rec, op)
        ref_pool, ref_t, _ = want[i]
        assert pool.tobytes() == ref_pool.tobytes(), i
        assert {k: totals[k] for k in ref_t} == ref_t, (i, totals, ref_t)
        assert totals["alive"] == totals["seeded"] + totals["spawned"] - totals["dropped"] - sum(totals[k] for k in ("diedLife", "diedAge", "leftBox", "nonFinite"))
        assert totals["crestSpawned"] <= totals["spawned"]
    assert totals["acting"] == len(range(0, D.SCENE_STEPS, every)) and totals["crestSpawned"] > 0


def test_the_scene_contains_every_event(pkg, oracle):
    snaps = K.scene_reference(pkg, oracle, K.ROOMY)
    evs = [s[2] for s in snaps]
    print("aligned shell members after substeps 0, 4, 12, 23:", [evs[i]["aligned"] for i in (0, 4, 12, 23)])
    print("events summed over the run:", {k: sum(e[k] for e in evs) for k in evs[0]})
    for key in ("crestBorn", "crestOnly", "both", "pc0", "pc1", "pk0", "pk1"):
        assert sum(e[key] for e in evs) > 0, key
    assert snaps[-1][1]["dropped"] == 0                                      # the large pool keeps every child ...
    small = K.scene_reference(pkg, oracle, 64)
    assert small[-1][1]["dropped"] > 0                                       # ... the small one does not
    third = K.scene_reference(pkg, oracle, K.ROOMY, 3)
    assert third[-1][1]["acting"] == 8 and 0 < third[-1][1]["crestSpawned"] < snaps[-1][1]["crestSpawned"]
    assert all(e == {} for i, (_, _, e) in enumerate(third) if i % 3)


def test_off_is_the_plain_host_step(pkg, oracle):
    rec, sp, op, pool = D.scene(pkg, oracle)
    cfg = pkg.diffuse_config(**D.SCENE_CONFIG)
    b = oracle.build_grid(rec, op)
    u, cnt = D.sample(rec, pool["pos"], op.h, op.mass, b["grid"], b["cell_start"], b["order"])
    smp = _samples(pkg, u, cnt)
    want, want_t = pkg.diffuse_step_host(cfg, sp, pool, smp, rec, 5)
    off = K.scene_crest(pkg, sp, rate=0.0)
    rows = K.shell_rows(pkg, rec, sp, K.scene_crest(pkg, sp))
    for crest, r in ((off, rows), (off, None)):
        got, t = pkg.diffuse_step_host(cfg, sp, pool, smp, rec, 5, crest=crest, shell_rows=r)
        assert got.tobytes() == want.tobytes() and {k: t[k] for k in want_t} == want_t
        assert (t["acting"], t["crestSpawned"], t["shellSize"]) == (0, 0, 0)
    # a substep on which the term does not act: the same bytes, the books stand
    got, t = pkg.diffuse_step_host(cfg, sp, pool, smp, rec, 5, crest=K.scene_crest(pkg, sp, every=4), shell_rows=rows)
    assert got.tobytes() == want.tobytes() and (t["acting"], t["crestSpawned"]) == (0, 0)
    # the L function itself with a null crest and null rows
    L = pkg.load_library()
    out = np.zeros(cfg.capacity, pkg.DIFFUSE_DTYPE)
    n = C.c_size_t()
    P = np.ascontiguousarray(rec, pkg.PARTICLE_DTYPE)
    assert L.sph_diffuse_step_host_crest(C.byref(cfg), None, C.byref(sp), -1.0, 5, pool.ctypes.data, len(pool), smp.ctypes.data, P.ctypes.data, len(P),
                                         None, out.ctypes.data, C.byref(n), None, None) == 0
    assert out[:n.value].tobytes() == want.tobytes()


def test_foam_children_are_what_they_were(pkg, oracle):
    rec, sp, op, _ = D.scene(pkg, oracle)
    cfg = pkg.diffuse_config(**dict(D.SCENE_CONFIG, capacity=65536, maxPerParent=8))
    crest = K.scene_crest(pkg, sp)
    rows = K.shell_rows(pkg, rec, sp, crest)
    plain, tp = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 0)
    both, tb = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 0, crest=crest, shell_rows=rows)
    f = np.bincount(plain["parent"], minlength=len(rec))
    a = np.bincount(both["parent"], minlength=len(rec))
    assert np.all(a >= f) and np.all(a <= 8) and tb["crestSpawned"] == int((a - f).sum()) > 0 and tb["spawned"] == tp["spawned"] + tb["crestSpawned"]
    assert ((a > f) & (f > 0)).any() and ((a > f) & (f == 0)).any()
    first = np.cumsum(a) - a
    k = np.arange(len(both)) - first[both["parent"]]                         # child number within its parent
    assert both[k < f[both["parent"]]].tobytes() == plain.tobytes()          # children 0 .. f - 1 are the foam term's, byte for byte
    assert list(both["parent"]) == sorted(both["parent"])


SIDE = 12


def _block(pkg, direction):
    rec, sp, nominal = shell_scenes.block(pkg, side=SIDE)
    rec = rec.copy()
    rec["density"], rec["padA"] = 1000.0, 0.0
    pos = rec["pos"][:, :3].astype(np.float64)
    rec["vel"][:, :3] = (direction * 5.0 * pos / np.linalg.norm(pos, axis=1)[:, None]).astype(F)
    return rec, sp, nominal


def test_where_births_come_from(pkg):
    cfg = pkg.diffuse_config(capacity=65536, threshold=0.5, maxPerParent=1)
    crest = pkg.diffuse_crest_config(rate=1e9, radius=0.0, offset=0.10, crestMin=0.25, crestMax=1.0, speedMin=1.0, speedMax=2.0)
    rec, sp, nominal = _block(pkg, 1.0)
    assert len(rec) == 1728
    rows = K.shell_rows(pkg, rec, sp, crest)
    out, t = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 0, crest=crest, shell_rows=rows)
    depth = np.sort((SIDE - 1) / 2.0 - np.abs(nominal), axis=1)            # the three face depths in spacings, ascending
    member = (rows["flags"] & pkg.SPH_SHELL_MEMBER) != 0
    parents = np.zeros(len(rec), bool)
    parents[out["parent"]] = True
    far, near = member & (depth[:, 1] > 3.0), member & (depth[:, 1] < 2.0)  # (near: in the two lattice layers next to an edge, 344 members)
    print(f"shell {member.sum()}, parents {parents.sum()}; far from every edge {far.sum()} (largest crest {rows['crest'][far].max():.3f}), "
          f"within 2 of an edge {near.sum()} of which parents {(near & parents).sum()}")
    assert t["spawned"] == t["crestSpawned"] == parents.sum() > 0 and t["shellSize"] == member.sum() and t["acting"] == 1
    assert far.sum() > 0 and not (parents & (depth[:, 1] > 3.0)).any()     # nobody is born on a flat face
    assert (near & parents).sum() >= 0.9 * near.sum() > 0                   # the edges and corners bear
    assert not (parents & ~member).any()
    for direction in (-1.0, 0.0):                                            # moving inward, or at rest: nobody
        rec, sp, _ = _block(pkg, direction)
        out, t = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, 0, crest=crest, shell_rows=rows)
        ok, _, _, _, aligned = K.potentials(rec, rows, crest)
        assert len(out) == 0 and t["crestSpawned"] == 0 and t["acting"] == 1 and not aligned.any() and not ok.any(), direction


def test_draw_33_and_window_known_answers(pkg):
    # hash(seed, id, counter, 33): the value worked out with section 3j, and the library's use of it
    assert int(D.hash32(0xFFFFFFFF, np.array([0xFFFFFFFF]), (1 << 40) + 5, np.array([33]))[0]) == 0xc9be4936
    assert list(K.window(np.array([0.0, 0.25, 0.4375, 1.0, 3.0], F), 0.25, 1.0)) == [0.0, 0.0, 0.25, 1.0, 1.0]
    assert list(K.window(np.array([-1.0, 10.0, 20.0, 30.0, 1e30], F), 10.0, 30.0)) == [0.0, 0.0, 0.5, 1.0, 1.0]
    sp = pkg.default_params()
    dt = 2.0 ** -10
    n = 64
    rec = np.zeros(n, pkg.PARTICLE_DTYPE)
    rec["density"] = 1000.0
    rows = np.zeros(n, pkg.SHELL_DTYPE)
    rows["flags"] = pkg.SPH_SHELL_MEMBER
    rows["normal"][:, 1] = 1.0
    cfg = pkg.diffuse_config(capacity=4096, seed=5, threshold=0.5, maxPerParent=8)

    def born(crest_value, speed, rate, counter=7):
        rec["vel"][:, :3] = (0.0, speed, 0.0)
        rows["crest"] = crest_value
        crest = pkg.diffuse_crest_config(rate=rate, crestMin=0.25, crestMax=1.0, speedMin=10.0, speedMax=30.0, align=0.6, every=1)
        out, t = pkg.diffuse_step_host(cfg, sp, D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), rec, counter, dt=dt, crest=crest, shell_rows=rows)
        cnt = np.bincount(out["parent"], minlength=n)
        assert t["crestSpawned"] == cnt.sum() == t["spawned"]
        return cnt
    # lam = 1/2 exactly (rate dt = 1/2, pc = pk = 1): one child iff U_33 >= 1/2
    u33 = D.uniform(5, np.arange(n), 7, 33)
    got = born(1.0, 30.0, 512.0)
    assert list(got) == list((u33 >= F(0.5)).astype(int)) and 0 < got.sum() < n
    u33 = D.uniform(5, np.arange(n), (1 << 33) + 2, 33)                     # the high word of the counter enters
    assert list(born(1.0, 30.0, 512.0, counter=(1 << 33) + 2)) == list((u33 >= F(0.5)).astype(int))
    # rate dt = 4: floor(4 pc pk + U) is 4 pc pk wherever that is whole -- at, below and above both ends of both windows
    for crest_value, speed, want in ((0.25, 30.0, 0), (0.2, 30.0, 0), (-1.0, 30.0, 0), (1.0, 30.0, 4), (1.5, 30.0, 4), (100.0, 30.0, 4),
                                     (1.0, 10.0, 0), (1.0, 9.0, 0), (1.0, 31.0, 4), (1.0, 1e6, 4), (1.0, 20.0, 2), (0.625, 30.0, 2),
                                     (0.625, 20.0, 1)):
        assert list(born(crest_value, speed, 4096.0)) == [want] * n, (crest_value, speed)
    # who does not qualify, each for one reason
    base = born(1.0, 30.0, 4096.0)
    assert list(base) == [4] * n
    rows["flags"][0] = 0
    rows["flags"][1] = pkg.SPH_SHELL_MEMBER | pkg.SPH_SHELL_ISOLATED
    rec["isGhost"][2] = 1
    rec["density"][3] = 0.0
    rows["normal"][4] = (0.0, -1.0, 0.0)                                      # moves against its normal
    rows["normal"][5] = (0.8, 0.6, 0.0)                                       # dot = 0.6 sp: exactly aligned
    rows["normal"][6] = (0.8, 0.59, 0.0)
    got = born(1.0, 30.0, 4096.0)
    assert list(got[:8]) == [0, 0, 0, 0, 0, 4, 0, 4]


BAD = (dict(rate=np.nan), dict(rate=-1.0), dict(rate=np.inf), dict(radius=np.nan), dict(radius=1e3), dict(offset=-0.1), dict(offset=np.nan),
       dict(crestMin=1.0, crestMax=1.0), dict(crestMin=2.0, crestMax=1.0), dict(crestMax=np.inf), dict(crestMin=np.nan),
       dict(speedMin=5.0, speedMax=5.0), dict(speedMax=np.nan), dict(align=-0.01), dict(align=1.01), dict(align=np.nan), dict(every=0),
       dict(flags=2))


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(d))
def test_crest_config_refusals(pkg, bad):
    crest = pkg.diffuse_crest_config(**bad)
    with pytest.raises(pkg.SphError, match="-1"):
        pkg.diffuse_step_host(pkg.diffuse_config(), pkg.default_params(), D.empty(), np.zeros(0, pkg.SAMPLE_DTYPE), np.zeros(0, pkg.PARTICLE_DTYPE), 0,
                              crest=crest, shell_rows=None)
