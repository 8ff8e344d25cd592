"""Triangle-mesh obstacles through signed distance lattices on the GPU (include/sph_abi.h "signed distance lattices").

sph_mesh_distance is compared byte for byte with its host twin and the numpy restatement tests/volume_ref.py; records and poses after
substeps with bound bodies are compared bit for bit with the oracle's substep followed by the restatement, impulses within the bound of
section 3e for a re-ordered fp64 sum (tests/obstacle_ref.py impulse_bound)."""
import re
import shutil

import numpy as np
import pytest

from conftest import assert_records_equal, small_scene, to_oracle_params
import obstacle_ref as R
import surface_ref as sr
import volume_ref as VR
from support import build_example, check_impulses, engine, fluid_block, run_example, same_bits

pytestmark = pytest.mark.gpu

F = np.float32


def mesh_fixtures():
    """(name, vertices, triangles, origin, spacing, dims): the lattices are offset so that no point lies on a surface."""
    out = []
    v, t = VR.icosphere(2, 1.0)
    out.append(("icosphere", v, t, (-1.4317, -1.4291, -1.4353), 0.1247, (24, 24, 24)))
    v, t = VR.cube(0.8)
    out.append(("cube", v, t, (-1.5131, -1.4977, -1.5213), 0.1593, (20, 20, 20)))
    a = (np.arange(14) - 6.5) * 0.2
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    f = (1.0 - (x * x / 1.1 ** 2 + y * y / 0.8 ** 2 + z * z / 0.9 ** 2) + 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y)).astype(F)
    pos, _, tris = sr.extract(f, (a[0], a[0], a[0]), (0.2, 0.2, 0.2), 0.0)
    out.append(("mesher", pos.astype(F), tris.astype(np.uint32), (-1.4519, -1.4633, -1.4471), 0.1811, (17, 17, 17)))
    return out


def _scene_bodies(pkg, rec, dt):
    """Volumes and bodies sized from the fluid block: a sphere lattice and a box lattice with a flat core."""
    c, E = fluid_block(rec)
    Rs = 0.2 * E
    hs = Rs / 6.0
    sphere = VR.sphere_lattice(Rs, hs)
    bh = (0.2 * E, 0.14 * E, 0.12 * E)
    hb = 0.12 * E / 5.0
    box = VR.box_lattice(bh, hb, floor=-0.06 * E)
    return c, E, (sphere, hs), (box, hb)


def _reference(oracle, rec, sp, arr, vols, bindings, steps):
    op = to_oracle_params(oracle, sp)
    bs = R.bodies(arr, normalise=True)
    rv = [VR.volume(v, h) for v, h in vols]
    out = []
    for _ in range(steps):
        rec, bs, imp, info = VR.step(oracle, rec, op, bs, rv, bindings)
        out.append((rec, R.to_array(bs), imp, info))
    return out


def _half(vh):
    return VR.volume(*vh)["half"]


def _scenarios(pkg, rec, dt):
    c, E, sph, box = _scene_bodies(pkg, rec, dt)
    move = tuple(0.04 * E / (8 * dt) * np.array([0.8, -0.5, 0.33]))
    spin = tuple(0.2 / (8 * dt) * np.array([0.3, 0.9, -0.3]))
    off = lambda x, y, z: (c + F(E) * np.array([x, y, z], F)).astype(F)
    return {
        "resting sphere lattice": ([pkg.obstacle(R.BOX, c, _half(sph))], [sph], [0]),
        "moving spinning box lattice": ([pkg.obstacle(R.BOX, c, _half(box), rotation=(0.9, 0.2, 0.3, 0.1), vel=move, omega=spin)], [box], [0]),
        "two bodies, one lattice": ([pkg.obstacle(R.BOX, off(-0.22, 0, 0), _half(sph), vel=move),
                                     pkg.obstacle(R.BOX, off(0.22, 0, 0), _half(sph), rotation=(0.8, -0.3, 0.1, 0.4), omega=spin)], [sph], [0, 0]),
        "primitive and volume": ([pkg.obstacle(R.CAPSULE, off(-0.22, 0, 0), (0.1 * E, 0.1 * E), omega=spin),
                                  pkg.obstacle(R.BOX, off(0.2, 0, 0), _half(box), vel=move)], [box], [-1, 0]),
        "box clips its lattice": ([pkg.obstacle(R.BOX, c, 0.7 * _half(sph), rotation=(0.9, 0.1, -0.2, 0.3), omega=spin)], [sph], [0]),
    }


def _bind_all(f, vols, bindings):
    ids = [f.create_volume(v, h) for v, h in vols]
    for i, b in enumerate(bindings):
        if b >= 0:
            f.bind_obstacle_volume(i, ids[b])
    return ids


def test_mesh_distance_equals_the_host_twin_and_the_restatement(pkg):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    f = engine(pkg, rec0, sp)
    for name, v, t, origin, h, dims in mesh_fixtures():
        want, w = VR.mesh_distance(v, t, origin, h, dims)
        dev = np.abs(w - np.round(w)).max()
        print(f"{name}: {len(t)} triangles, {want.size} points, max |w - round(w)| = {dev:.3g}, {int((want < 0).sum())} inside")
        assert dev < 0.01 and (want < 0).any() and (want > 0).any()
        host = pkg.mesh_distance_host(v, t, origin, h, dims)
        same_bits(host, want, f"{name}: host twin against the restatement")
        for split in (0, 1, 2, 5):
            f.set_option(pkg.SPH_OPT_MESH_SPLIT, split)
            got = f.mesh_distance(v, t, origin, h, dims).cpu().numpy()
            same_bits(got, want, f"{name}: split {split}")
    f.close()


def test_mesh_distance_large_case_does_not_depend_on_the_split(pkg):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    f = engine(pkg, rec0, sp)
    RADIUS = 0.27                                                       # about six spacings: the near-surface set stays a few thousand points
    v, t = VR.icosphere(5, RADIUS)
    assert len(t) == 20480
    n, h = 64, F(0.0437)
    origin = np.array([-1.3771, -1.3693, -1.3817], F)
    outs = []
    for split in (3, 16, 0):
        f.set_option(pkg.SPH_OPT_MESH_SPLIT, split)
        outs.append(f.mesh_distance(v, t, origin, h, (n, n, n)).cpu().numpy())
    same_bits(outs[0], outs[1], "split 3 against split 16")
    same_bits(outs[0], outs[2], "split 3 against the engine's choice")
    got = outs[0]
    pts = VR.lattice_points(origin, h, (n, n, n)).astype(np.float64)
    r = np.linalg.norm(pts, axis=1)
    edge = np.linalg.norm(v[t[:, 0]].astype(np.float64) - v[t[:, 1]].astype(np.float64), axis=1).max()
    sag = RADIUS - np.sqrt(RADIUS ** 2 - (edge / np.sqrt(3.0)) ** 2)          # the circumradius of a face is at most edge / sqrt(3)
    near = np.nonzero(np.abs(r - RADIUS) <= 2.0 * float(h) + sag)[0]
    rng = np.random.default_rng(5)
    pick = np.unique(np.concatenate([near, rng.choice(n ** 3, 1500, replace=False)]))
    print(f"{len(near)} points within two spacings of the surface, {len(pick)} compared; sagitta {sag:.3g}")
    assert len(near) > 500
    # the host twin computes lattices: point (i, j, k) is the 1 x 1 x 1 lattice that starts at it (origin + 0 * spacing is exact)
    flat = got.ravel()
    axes = [(origin[a] + (np.arange(n).astype(F) * h).astype(F)).astype(F) for a in range(3)]
    bad = 0
    for p in pick:
        i, j, k = p % n, (p // n) % n, p // (n * n)
        one = pkg.mesh_distance_host(v, t, (axes[0][i], axes[1][j], axes[2][k]), h, (1, 1, 1)).ravel()[0]
        bad += int(one.tobytes() != flat[p].tobytes())
    assert bad == 0, f"{bad} of {len(pick)} points differ from the host twin"
    assert (np.abs(flat.astype(np.float64) - (r - RADIUS)) <= sag + 1e-5).all()
    f.close()


def test_round_trip_through_the_mesher(pkg):
    import torch
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    f = engine(pkg, rec0, sp)
    name, v, t, origin, h, dims = mesh_fixtures()[0]
    phi = f.mesh_distance(v, t, origin, h, dims)
    mv, mt = f.surface_from_volume((-phi).contiguous(), origin, (h, h, h), None, 0.0)
    assert len(mt) > 100 and sr.closed_oriented(mt)
    vol = sr.enclosed_volume(mv["pos"], mt)
    edge = np.linalg.norm(v[t[:, 0]].astype(np.float64) - v[t[:, 1]].astype(np.float64), axis=1).max()
    sag = 1.0 - np.sqrt(1.0 - (edge / np.sqrt(3.0)) ** 2)
    # the mesh lies between the spheres of radius 1 - sagitta and 1; the mesher moves a surface by less than one spacing
    lo, hi = 4.0 / 3.0 * np.pi * (1.0 - sag - h) ** 3, 4.0 / 3.0 * np.pi * (1.0 + h) ** 3
    print(f"enclosed volume {vol:.4f} in [{lo:.4f}, {hi:.4f}] (4/3 pi = {4.0 / 3.0 * np.pi:.4f}), sagitta {sag:.4f}")
    assert lo <= vol <= hi
    f.close()


@pytest.mark.parametrize("n,grid", ((4096, 16), (32768, 32)))
def test_parity_with_oracle_and_reference(pkg, oracle, n, grid):
    rec0, sp = small_scene(pkg, n=n, grid=grid)
    n_fluid = int((rec0["isGhost"] == 0).sum())
    dt = float(sp.param_timeStep)
    steps = 6
    for name, (obs, vols, bindings) in _scenarios(pkg, rec0, dt).items():
        arr = pkg.obstacle_array(obs)
        ref = _reference(oracle, rec0, sp, arr, vols, bindings, steps)
        for k, (_, _, _, info) in enumerate(ref):
            touched, neg = int(info["touched"].sum()), int(info["negative"].sum())
            assert touched >= 0.005 * n_fluid and neg >= 1, f"{n} {name} substep {k}: the reference touches {touched} of {n_fluid} ({neg} with u_n < 0)"
        print(f"{n} {name}: reference touches {[int(i['touched'].sum()) for _, _, _, i in ref]} of {n_fluid}")
        for kern, aos in ((3, 1), (3, 0), (2, 1), (1, 0)) if n > 4096 else [(k, a) for k in (1, 2, 3) for a in (0, 1)]:
            what = f"{n}: {name} pass {kern} aos {aos}"
            f = engine(pkg, rec0, sp, kern, aos)
            f.set_obstacles(arr)
            _bind_all(f, vols, bindings)
            for k, (want_rec, want_bodies, want_imp, info) in enumerate(ref):
                f.DispatchCompute()
                assert_records_equal(f.download(), want_rec, f"{what} substep {k}")
                same_bits(f.obstacles(), want_bodies, f"{what} substep {k}: poses")
                J, t, s = f.obstacle_impulses(reset=True)
                assert s == 1
                check_impulses(J, want_imp, info, f"{what} substep {k}")
            f.close()


def test_graph_replay_sees_bind_and_set_motion(pkg):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    c, E, sph, box = _scene_bodies(pkg, rec0, dt)
    arr = pkg.obstacle_array([pkg.obstacle(R.BOX, (c + F(E) * np.array([-0.2, 0, 0], F)), _half(sph)),
                              pkg.obstacle(R.BOX, (c + F(E) * np.array([0.2, 0, 0], F)), _half(box), rotation=(0.9, 0.2, 0.3, 0.1))])
    motions = [((1.0, 0.0, 0.0), (0.0, 2.0, 0.0)), ((0.0, -2.0, 0.5), (3.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((-1.5, 0.0, 1.0), (0.0, -4.0, 1.0))]
    runs = []
    for graph in (1, 0):
        f = engine(pkg, rec0, sp, 3, 1, graph)
        f.set_obstacles(arr)
        ids = [f.create_volume(*sph), f.create_volume(*box)]
        f.bind_obstacle_volume(0, ids[0])
        seen = []
        for i, (v, w) in enumerate(motions):
            f.DispatchN(16)
            seen.append((f.download(), f.obstacles(), f.obstacle_impulses(reset=i % 2 == 1)))
            f.set_obstacle_motion(i % 2, v, w)
            if i == 1:
                f.bind_obstacle_volume(1, ids[1])                          # (the same kernel: the replayed graph must see it)
            if i == 2:
                f.bind_obstacle_volume(0, -1)
        f.DispatchN(16)
        seen.append((f.download(), f.obstacles(), f.obstacle_impulses()))
        assert (f.obstacle_volume(0), f.obstacle_volume(1)) == (-1, ids[1])
        launches = f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
        runs.append(seen)
        f.close()
        if graph:
            assert launches > 0
    for k, ((ra, oa, ja), (rb, ob, jb)) in enumerate(zip(*runs)):
        assert_records_equal(ra, rb, f"call {k}: records")
        same_bits(oa, ob, f"call {k}: poses")
        same_bits(ja[0], jb[0], f"call {k}: impulses")
        assert ja[1:] == jb[1:]
    # a bind changes the result: the same calls without the second bind differ
    assert (runs[0][-1][2][0] != 0).any()


def test_sphere_lattice_against_the_analytic_sphere(pkg, oracle):
    """The tolerance is measured, not chosen: the relative difference of |J| between the two bodies on the restatement, times two."""
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    c, E, sph, _ = _scene_bodies(pkg, rec0, dt)
    Rs = 0.2 * E
    V = (0.04 * E / (8 * dt), 0.0, 0.0)
    body_v = pkg.obstacle_array([pkg.obstacle(R.BOX, c, _half(sph), vel=V)])
    body_s = pkg.obstacle_array([pkg.obstacle(R.SPHERE, c, Rs, vel=V)])
    steps = 8
    ref_v = _reference(oracle, rec0, sp, body_v, [sph], [0], steps)
    ref_s = _reference(oracle, rec0, sp, body_s, [], [-1], steps)
    Jv, Js = sum(x[2][0, :3] for x in ref_v), sum(x[2][0, :3] for x in ref_s)
    rel_cpu = np.linalg.norm(Jv - Js) / np.linalg.norm(Js)
    out = []
    for arr, bind in ((body_v, True), (body_s, False)):
        f = engine(pkg, rec0, sp)
        f.set_obstacles(arr)
        if bind:
            f.bind_obstacle_volume(0, f.create_volume(*sph))
        for _ in range(steps):
            f.DispatchCompute()
        out.append(f.obstacle_impulses()[0][0, :3])
        f.close()
    rel_gpu = np.linalg.norm(out[0] - out[1]) / np.linalg.norm(out[1])
    print(f"relative difference of |J| lattice against sphere: restatement {rel_cpu:.4g}, engine {rel_gpu:.4g}")
    assert np.linalg.norm(Js) > 0 and rel_gpu <= 2.0 * rel_cpu


def test_without_a_binding_nothing_changes(pkg):
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    c, E, sph, box = _scene_bodies(pkg, rec0, dt)
    arr = pkg.obstacle_array([pkg.obstacle(R.BOX, c, _half(box), rotation=(0.9, 0.2, 0.3, 0.1), omega=(0.0, 3.0, 0.0)),
                              pkg.obstacle(R.SPHERE, c + F(0.25 * E), 0.1 * E)])
    runs = []
    for mode in ("plain", "unbound", "bound"):
        f = engine(pkg, rec0, sp)
        f.set_option(pkg.SPH_OPT_TIMING, 1)
        f.set_obstacles(arr)
        if mode != "plain":
            vid = f.create_volume(*box)
            f.bind_obstacle_volume(0, vid)
        if mode == "unbound":
            f.set_obstacles(arr)                                       # a set clears the binding ...
            assert f.obstacle_volume(0) == -1
            f.bind_obstacle_volume(0, vid)
            f.bind_obstacle_volume(0, -1)                              # ... and so does an unbind
            f.destroy_volume(vid)
        f.DispatchN(6)
        runs.append((f.download(), f.obstacles(), f.obstacle_impulses()[0], {k: v[1] for k, v in f.kernel_times().items()}))
        f.close()
    assert_records_equal(runs[0][0], runs[1][0], "unbound against plain")
    same_bits(runs[0][1], runs[1][1], "poses")
    same_bits(runs[0][2], runs[1][2], "impulses")
    assert runs[0][3] == runs[1][3], (runs[0][3], runs[1][3])
    assert runs[0][3] == runs[2][3], "a bound body launches as many kernels per class"
    assert runs[2][0].tobytes() != runs[0][0].tobytes()


def test_refusals_on_the_device_path(pkg):
    import ctypes as C
    from importlib import import_module
    L = pkg.load_library()
    rec0, sp = small_scene(pkg, n=4096, grid=16)
    dt = float(sp.param_timeStep)
    c, E, sph, box = _scene_bodies(pkg, rec0, dt)
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec0, np.arange(len(rec0), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec0) * 1.2) + 8192)
    vals = np.ascontiguousarray(sph[0])
    dims = (C.c_int * 3)(vals.shape[2], vals.shape[1], vals.shape[0])
    sp3 = (C.c_float * 3)(sph[1], sph[1], sph[1])
    vid = C.c_int(-7)
    assert L.sph_volume_create(slab._h, vals.ctypes.data_as(C.c_void_p), dims, sp3, 0, C.byref(vid)) == -3 and b"slab" in L.sph_last_error()
    assert L.sph_obstacles_bind_volume(slab._h, 0, 0) == -3 and vid.value == -7
    slab.close()
    f = engine(pkg, rec0, sp)
    f.set_obstacles([pkg.obstacle(R.BOX, c, _half(sph)), pkg.obstacle(R.SPHERE, c, 0.1 * E)])
    a = f.create_volume(*sph)
    f.bind_obstacle_volume(0, a)
    for idx, v in ((1, a), (2, a), (-1, a), (0, 5), (0, 16), (0, 99)):
        with pytest.raises(pkg.SphError, match="-1"):
            f.bind_obstacle_volume(idx, v)
    assert (f.obstacle_volume(0), f.obstacle_volume(1)) == (a, -1)
    with pytest.raises(pkg.SphError, match="-3"):
        f.destroy_volume(a)
    for bad in (-1, 3, 16):
        with pytest.raises(pkg.SphError, match="-1"):
            f.destroy_volume(bad)
    with pytest.raises(pkg.SphError, match="-1"):
        f.create_volume(np.zeros((1, 4, 4), F), 0.1)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.SphError, match="-1"):
            f.create_volume(sph[0], h)
    more = [f.create_volume(np.zeros((2, 2, 2), F), 1.0) for _ in range(15)]
    assert sorted(more + [a]) == list(range(16))
    with pytest.raises(pkg.SphError, match="-4"):
        f.create_volume(np.zeros((2, 2, 2), F), 1.0)
    d, s, hf = f.volume_info(a)
    assert d == sph[0].shape[::-1] and np.array_equal(hf, _half(sph))
    f.DispatchN(2)                                                      # the bound body still works
    assert f.obstacle_impulses()[2] == 2
    f.bind_obstacle_volume(0, -1)
    f.destroy_volume(a)
    assert f.create_volume(*box) == a                                   # the slot is free again
    v, t = VR.cube(0.5)
    for vv, tt in ((v, np.array([[0, 1, 8]], np.uint32)), (np.where(np.arange(24).reshape(8, 3) == 4, np.nan, v).astype(F), t), (v, t[:0])):
        with pytest.raises(pkg.SphError, match="-1"):
            f.mesh_distance(vv, tt, (-1, -1, -1), 0.2, (8, 8, 8))
    f.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_mesh_obstacle_example_keeps_the_fluid_outside(pkg, tmp_path):
    res = run_example(build_example(pkg, "mesh_obstacle", tmp_path), ["200"], timeout=300)
    assert res.returncode == 0 and "mesh_obstacle OK" in res.stdout
    assert len(re.findall(r"torque=", res.stdout)) >= 10
