"""Signed distance lattices without a GPU: the host entry points (sph_volume_sample_host, sph_obstacles_apply_host_volumes,
sph_mesh_distance_host: the same __host__ __device__ functions the kernels run) against the numpy restatement tests/volume_ref.py.

Bounds used below and where they come from:
* Impulses: as in tests/test_obstacles_cpu.py (two fp64 sums of the same terms in different orders, obstacle_ref.impulse_bound).
* Residual of the projection: DESIGN.md section 3f fixes two unit-normal steps; on the lattice of |x| - 10 spacings the largest |phi| at a
  projected point must stay below 0.02 spacings (the figure the feature was specified with; measured 0.0076).
* Lattice sphere against the analytic sphere, normal direction: the trilinear interpolant of a distance field of curvature 1 / R differs
  from it by at most h^2 / (8 R) per axis (the sagitta of a chord of length h), 3 h^2 / (8 R) for three axes, plus the residual.
* The same, tangential direction: the interpolant's gradient is a blend of differences inside one cell, so it is the true gradient x / |x| at
  some point of that cell, at most sqrt(3) h away; seen from a particle at radius r that is an angle of at most atan(sqrt(3) h / (r - sqrt(3) h)),
  and the first step (length R - r) carries it sideways by (R - r) tan(angle).  Near the centre (r <= 2 sqrt(3) h) the direction is free
  and only the normal bound applies.
* Mesh distance against an fp64 brute force: d = sqrtf(dot3(e, e)), e = p - q.  q comes out of about ten rounded operations on numbers
  of size |x| + extent (dots, a quotient, a + t ab), so |q - q64| <= 10 * 2^-24 (|x| + extent) per component with a quotient that can
  amplify by at most one more factor of two; the dot and the root add 2 ulps of d: in all 32 * 2^-24 (|x| + extent).
"""
import ctypes as C

import numpy as np

import obstacle_ref as R
import surface_ref as sr
import volume_ref as VR
from support import check_impulses, records, same_bits

F = np.float32
U = 2.0 ** -24
VOLUME_SYMBOLS = ("sph_volume_create", "sph_volume_destroy", "sph_volume_info", "sph_volume_sample_host", "sph_volume_from_mesh",
                  "sph_obstacles_bind_volume", "sph_obstacles_volume", "sph_obstacles_apply_host_volumes", "sph_mesh_distance", "sph_mesh_distance_host")


def _sample_all(pkg, values, spacing, pts):
    out = [pkg.volume_sample_host(values, spacing, p) for p in pts]
    return np.array([o[0] for o in out], F), np.array([o[1] for o in out], F), np.array([o[2] for o in out], bool)


def test_library_exports_the_volume_interface(pkg):
    L = pkg.load_library()
    for name in VOLUME_SYMBOLS:
        assert hasattr(L, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.SphVolumeHost) == 32 and pkg.SPH_MAX_VOLUMES == 16 and L.sph_abi_version() == 4
    assert C.sizeof(pkg.SphObstacle) == 76
    for m in ("create_volume", "destroy_volume", "bind_obstacle_volume", "obstacle_volume", "mesh_distance", "volume_from_mesh", "volume_info"):
        assert hasattr(pkg.SPHFluidGPU, m), m


def test_sample_equals_the_restatement(pkg):
    rng = np.random.default_rng(21)
    for shape, spacing in (((7, 6, 5), (0.3, 0.2, 0.25)), ((2, 2, 2), (1.0, 1.0, 1.0)), ((4, 9, 3), (0.013, 2.5, 0.7))):
        values = rng.standard_normal(shape).astype(F)
        vol = VR.volume(values, spacing)
        half = vol["half"]
        pts = (rng.uniform(-1.15, 1.15, (600, 3)) * half).astype(F)
        axes = [(np.arange(vol["dims"][a]).astype(F) * vol["spacing"][a] - half[a]).astype(F) for a in range(3)]
        on_planes = pts[:120].copy()
        for i, p in enumerate(on_planes):
            a = i % 3
            p[a] = axes[a][rng.integers(len(axes[a]))]
        faces = pts[120:180].copy()
        for i, p in enumerate(faces):
            p[i % 3] = half[i % 3] * (1 if i % 2 else -1)
        nans = pts[180:190].copy()
        nans[np.arange(10), np.arange(10) % 3] = np.nan
        corners = np.array([[sx * half[0], sy * half[1], sz * half[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], F)
        allp = np.concatenate([pts, on_planes, faces, nans, corners, np.nextafter(corners, F(np.inf) * np.sign(corners)).astype(F)])
        want = VR.sample_host_result(vol, allp)
        got = _sample_all(pkg, values, spacing, allp)
        for g, w, name in zip(got, want, ("phi", "gradient", "inside")):
            same_bits(g, w, f"{shape}: {name}")
        assert want[2].any() and (~np.isnan(want[0])).sum() > 300 and np.isnan(want[0]).sum() > 50
        # NaN corners: every compare is false
        holed = values.copy()
        holed[shape[0] // 2, shape[1] // 2, shape[2] // 2] = np.nan
        vh = VR.volume(holed, spacing)
        want = VR.sample_host_result(vh, pts)
        got = _sample_all(pkg, holed, spacing, pts)
        for g, w, name in zip(got, want, ("phi", "gradient", "inside")):
            same_bits(g, w, f"{shape} with a NaN corner: {name}")
        assert np.isnan(want[0][want[1][:, 0] != want[1][:, 0]]).all() and not want[2][np.isnan(want[0])].any()


def test_sample_of_a_linear_function_is_exact_to_rounding(pkg):
    a, b = np.array([0.7, -1.3, 0.45]), 0.2
    n, h = (9, 8, 7), (0.25, 0.5, 0.125)
    ax = [(np.arange(n[i]) - 0.5 * (n[i] - 1)) * h[i] for i in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    values = (a[0] * x + a[1] * y + a[2] * z + b).astype(F)
    vol = VR.volume(values, h)
    rng = np.random.default_rng(4)
    pts = (rng.uniform(-1, 1, (500, 3)) * vol["half"]).astype(F)
    phi, grad, _ = _sample_all(pkg, values, h, pts)
    exact = pts.astype(np.float64) @ a + b
    scale = np.abs(values).max()
    # lattice values carry half an ulp each, the coordinate two roundings, seven lerps three roundings each
    assert np.abs(phi - exact).max() <= 32 * U * scale
    # a difference of two values rounded to half an ulp of `scale`, divided by the spacing
    assert (np.abs(grad - a) <= 8 * U * scale / np.array(h)).all()


def _lattice_scene(pkg, rng, bodies, n=6000, spread=1.6):
    lo = np.min([np.asarray(b.center) - spread for b in bodies], axis=0)
    hi = np.max([np.asarray(b.center) + spread for b in bodies], axis=0)
    pos = rng.uniform(lo, hi, (n, 3)).astype(F)
    vel = (rng.standard_normal((n, 3)) * 2.0).astype(F)
    ghost = (rng.uniform(size=n) < 0.05).astype(np.int32)
    pos[:5, 0] = np.nan
    return records(pkg, pos, vel, ghost)


def test_apply_equals_the_restatement(pkg):
    rng = np.random.default_rng(33)
    q = R.normalize(np.array([0.9, 0.2, 0.3, 0.1], F))
    sphere = (VR.sphere_lattice(1.0, 0.125), 0.125)
    box = (VR.box_lattice((0.9, 0.6, 0.5), 0.1, floor=-0.25), 0.1)
    hs, hb = VR.volume(*sphere)["half"], VR.volume(*box)["half"]
    cases = {
        "sphere lattice": ([pkg.obstacle(R.BOX, (0.1, 0.2, -0.1), hs)], [sphere], [0]),
        "box lattice with a flat core": ([pkg.obstacle(R.BOX, (0.0, 0.0, 0.0), hb)], [box], [0]),
        "rotated and moving": ([pkg.obstacle(R.BOX, (0.3, -0.2, 0.1), hb, rotation=q, vel=(1.0, -2.0, 0.5), omega=(0.5, 3.0, -1.0), restitution=0.4, friction=0.3)],
                               [box], [0]),
        "a primitive, then a volume": ([pkg.obstacle(R.CAPSULE, (-0.5, 0.0, 0.0), (0.5, 0.6), rotation=q, omega=(0, 2, 0)),
                                        pkg.obstacle(R.BOX, (0.6, 0.1, 0.0), hs, vel=(0.0, 1.0, 0.0))], [box, sphere], [-1, 1]),
        "a box that clips its lattice": ([pkg.obstacle(R.BOX, (0.0, 0.0, 0.0), (0.7 * hs[0], 0.5 * hs[1], hs[2]), rotation=q)], [sphere], [0]),
    }
    for name, (obs, vols, bindings) in cases.items():
        arr = pkg.obstacle_array(obs)
        rec = _lattice_scene(pkg, rng, obs)
        bs = R.bodies(arr, normalise=False)
        want, imp, info = VR.apply(bs, [VR.volume(*v) for v in vols], bindings, F(0.02), rec)
        got, J = pkg.obstacles_apply_host_volumes(arr, vols, bindings, 0.02, rec)
        same_bits(got, want, f"{name}: records")
        check_impulses(J, imp, info, name)
        assert info["touched"].min() >= 50 and info["negative"].min() >= 10, (name, info["touched"], info["negative"])
        plain, Jp = pkg.obstacles_apply_host(arr, 0.02, rec)
        assert plain.tobytes() != got.tobytes(), f"{name}: the volume changes nothing"
        none, Jn = pkg.obstacles_apply_host_volumes(arr, vols, [-1] * len(arr), 0.02, rec)
        same_bits(none, plain, f"{name}: without bindings")
        same_bits(Jn, Jp, f"{name}: impulses without bindings")
    # the flat core of the box lattice sends particles to the box's own faces: the fallback must have been taken
    vol = VR.volume(*box)
    how, _, _ = VR.project(vol, (rng.uniform(-0.3, 0.3, (2000, 3))).astype(F))
    assert (how == 2).sum() > 100


def test_projection_residual_and_agreement_with_the_analytic_sphere(pkg):
    Rs, h = 10.0, 1.0
    values = VR.sphere_lattice(Rs, h, margin=6)
    assert values.shape == (33, 33, 33)
    vol = VR.volume(values, h)
    rng = np.random.default_rng(11)
    pos = rng.uniform(-10.0, 10.0, (200000, 3)).astype(F)
    rec = records(pkg, pos, np.zeros_like(pos))
    body_v = R.bodies(pkg.obstacle_array([pkg.obstacle(R.BOX, (0, 0, 0), vol["half"])]), normalise=False)
    body_s = R.bodies(pkg.obstacle_array([pkg.obstacle(R.SPHERE, (0, 0, 0), Rs)]), normalise=False)
    out_v, _, info_v = VR.apply(body_v, [vol], [0], F(0.02), rec)
    out_s, _, info_s = R.apply(body_s, F(0.02), rec)
    moved = (out_v["pos"][:, :3] != rec["pos"][:, :3]).any(axis=1)
    assert info_v["touched"][0] > 100000 and moved.sum() == info_v["touched"][0]
    p = out_v["pos"][moved, :3]
    phi, _, within = VR.sample(vol, p)
    residual = np.abs(phi).max() / h
    print(f"{moved.sum()} inside points of {len(pos)}: max |phi(p')| = {residual:.4g} spacings after one application")
    assert within.all() and residual <= 0.02
    # normal direction: on the analytic sphere's surface within the chord of three axes plus the residual
    r1 = np.linalg.norm(p.astype(np.float64), axis=1)
    normal_bound = 3.0 * h * h / (8.0 * Rs) + 0.02 * h
    print(f"max | |p'| - R | = {np.abs(r1 - Rs).max():.4g}, bound {normal_bound:.4g}")
    assert np.abs(r1 - Rs).max() <= normal_bound
    # full position against SPH_OBSTACLE_SPHERE: the sideways offset of the first step, see the module docstring
    both = moved & (out_s["pos"][:, :3] != rec["pos"][:, :3]).any(axis=1)
    r0 = np.linalg.norm(rec["pos"][both, :3].astype(np.float64), axis=1)
    k = np.sqrt(3.0) * h
    far = r0 > 2.0 * k
    diff = np.linalg.norm(out_v["pos"][both, :3].astype(np.float64) - out_s["pos"][both, :3].astype(np.float64), axis=1)
    bound = (Rs - r0[far]) * np.tan(np.arctan(k / (r0[far] - k))) + normal_bound
    print(f"{far.sum()} particles beyond 2 sqrt(3) h of the centre: max position difference / bound = {(diff[far] / bound).max():.3g}")
    assert far.sum() > 90000 and (diff[far] <= bound).all()


def _mesh_cases():
    v, t = VR.icosphere(2, 1.0)
    yield "icosphere", v, t, (-1.4317, -1.4291, -1.4353), 0.1247, (24, 24, 24)
    v, t = VR.cube(0.8)
    yield "cube", v, t, (-1.5131, -1.4977, -1.5213), 0.1593, (20, 20, 20)
    a = (np.arange(14) - 6.5) * 0.2
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    f = (1.0 - (x * x / 1.1 ** 2 + y * y / 0.8 ** 2 + z * z / 0.9 ** 2) + 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y)).astype(F)
    pos, _, tris = sr.extract(f, (a[0], a[0], a[0]), (0.2, 0.2, 0.2), 0.0)
    assert sr.closed_oriented(tris)
    yield "mesher", pos.astype(F), tris.astype(np.uint32), (-1.4519, -1.4633, -1.4471), 0.1811, (17, 17, 17)


def test_mesh_distance_equals_the_restatement(pkg):
    for name, v, t, origin, h, dims in _mesh_cases():
        want, w = VR.mesh_distance(v, t, origin, h, dims)
        dev = np.abs(w - np.round(w)).max()
        print(f"{name}: {len(t)} triangles, {want.size} points, max |w - round(w)| = {dev:.3g}, {int((want < 0).sum())} inside")
        assert dev < 0.01, f"{name}: a lattice point lies on the surface"
        got = pkg.mesh_distance_host(v, t, origin, h, dims)
        same_bits(got, want, name)                                       # every point
        assert (want < 0).sum() > 100 and (want > 0).sum() > 100
        assert np.array_equal(want < 0, (np.round(w) == 1).reshape(want.shape))
        pts = VR.lattice_points(origin, h, dims)
        d64 = VR.brute_distance64(v, t, pts)
        extent = np.abs(v).max()
        bound = 32 * U * (np.abs(pts).max(axis=1) + extent)
        err = np.abs(np.abs(want.ravel()).astype(np.float64) - d64)
        print(f"{name}: max |d - d64| = {err.max():.3g}, smallest bound {bound.min():.3g}")
        assert (err <= bound).all()
        if name == "icosphere":
            assert len(t) >= 320
            edge = np.linalg.norm(v[t[:, 0]].astype(np.float64) - v[t[:, 1]].astype(np.float64), axis=1).max()
            sag = 1.0 - np.sqrt(1.0 - (edge / np.sqrt(3.0)) ** 2)          # a face's circumradius is at most edge / sqrt(3)
            r = np.linalg.norm(pts.astype(np.float64), axis=1)
            off = want.ravel().astype(np.float64) - (r - 1.0)
            print(f"icosphere: phi - (|x| - R) in [{off.min():.4g}, {off.max():.4g}], sagitta {sag:.4g}")
            assert off.min() >= -1e-6 and off.max() <= sag + 1e-6
        if name == "cube":
            # the lattice has points in the vertex, edge and face regions of the cube
            a = np.abs(pts.astype(np.float64))
            beyond = (a > 0.8).sum(axis=1)
            assert (beyond == 3).any() and (beyond == 2).any() and (beyond == 1).any()
    # a mesh wound the other way is outside everywhere
    v, t = VR.cube(0.8)
    flipped = pkg.mesh_distance_host(v, t[:, ::-1], (-1.5131, -1.4977, -1.5213), 0.1593, (20, 20, 20))
    assert (flipped > 0).all()


def test_refusals_write_nothing(pkg):
    L = pkg.load_library()
    values = VR.sphere_lattice(1.0, 0.25)
    vf = np.ascontiguousarray(values)
    n = values.shape[0]
    local = (C.c_float * 3)(0.1, 0.2, 0.3)

    def sample(dims, spacing, vals=vf):
        phi, inside, g = C.c_float(77.0), C.c_int(7), (C.c_float * 3)(5, 5, 5)
        rc = L.sph_volume_sample_host(vals.ctypes.data_as(C.c_void_p) if vals is not None else None, (C.c_int * 3)(*dims), (C.c_float * 3)(*spacing), local,
                                      C.byref(phi), g, C.byref(inside))
        assert (phi.value, inside.value, list(g)) == (77.0, 7, [5, 5, 5]) or rc == 0
        return rc
    assert sample((n, n, n), (0.25,) * 3) == 0
    for dims, spacing in (((1, n, n), (0.25,) * 3), ((n, n, 0), (0.25,) * 3), ((65536, 65536, 2), (0.25,) * 3), ((n, n, n), (0.0, 0.25, 0.25)),
                          ((n, n, n), (0.25, -1.0, 0.25)), ((n, n, n), (0.25, 0.25, float("nan"))), ((n, n, n), (float("inf"), 0.25, 0.25))):
        assert sample(dims, spacing) == -1, (dims, spacing)
    assert sample((n, n, n), (0.25,) * 3, None) == -1
    half = VR.volume(values, 0.25)["half"]
    rng = np.random.default_rng(2)
    box = pkg.obstacle(R.BOX, (0, 0, 0), half)
    rec = records(pkg, rng.uniform(-1.5, 1.5, (500, 3)).astype(F), rng.standard_normal((500, 3)).astype(F))
    ok, _ = pkg.obstacles_apply_host_volumes([box], [(values, 0.25)], [0], 0.02, rec)
    assert ok.tobytes() != rec.tobytes()
    arr = pkg.obstacle_array([box])
    vols = (pkg.SphVolumeHost * 2)()
    for v in vols:
        v.values, v.dims[:], v.spacing[:] = vf.ctypes.data, [n, n, n], [0.25] * 3

    def apply(obs, count, nvol, bind, volumes=vols):
        r = rec.copy()
        imp = np.full((2, 6), 9.0)
        b = np.asarray(bind, np.int32)
        rc = L.sph_obstacles_apply_host_volumes(obs.ctypes.data_as(C.c_void_p), count, C.byref(volumes) if volumes is not None else None, nvol,
                                                b.ctypes.data_as(C.c_void_p), C.c_float(0.02), r.ctypes.data_as(C.c_void_p), len(r), imp.ctypes.data_as(C.c_void_p))
        if rc != 0:
            assert r.tobytes() == rec.tobytes() and (imp == 9.0).all(), "a refused call wrote something"
        return rc
    assert apply(arr, 1, 1, [0]) == 0
    assert apply(arr, 1, 1, [1]) == -1                                   # a binding beyond the volumes
    assert apply(arr, 1, 17, [0]) == -1 and apply(arr, 1, -1, [0]) == -1 and apply(arr, 17, 1, [0] * 17) == -1
    assert apply(arr, 1, 1, [0], None) == -1
    for shape, size in ((R.SPHERE, (1.0,)), (R.CAPSULE, (0.5, 0.5))):
        assert apply(pkg.obstacle_array([pkg.obstacle(shape, (0, 0, 0), size)]), 1, 1, [0]) == -1      # only a box can be bound
        assert apply(pkg.obstacle_array([pkg.obstacle(shape, (0, 0, 0), size)]), 1, 1, [-1]) == 0
    bad = (pkg.SphVolumeHost * 2)()
    bad[0].values, bad[0].dims[:], bad[0].spacing[:] = vf.ctypes.data, [n, 1, n], [0.25] * 3
    assert apply(arr, 1, 1, [0], bad) == -1
    bad[0].dims[:], bad[0].spacing[:] = [n, n, n], [0.25, 0.0, 0.25]
    assert apply(arr, 1, 1, [0], bad) == -1
    bad[0].values, bad[0].spacing[:] = None, [0.25] * 3
    assert apply(arr, 1, 1, [0], bad) == -1
    assert apply(pkg.obstacle_array([pkg.obstacle(3, (0, 0, 0), half)]), 1, 1, [-1]) == -1          # shape 3 stays unknown
    # mesh distance
    v, t = VR.cube(0.5)
    out = np.full(8, 3.0, F)

    def mesh(vv, tt, origin=(-1, -1, -1), spacing=(1, 1, 1), dims=(2, 2, 2), nv=None):
        vv, tt = np.ascontiguousarray(vv, F), np.ascontiguousarray(tt, np.uint32)
        rc = L.sph_mesh_distance_host(vv.ctypes.data_as(C.c_void_p), len(vv) if nv is None else nv, tt.ctypes.data_as(C.c_void_p), len(tt),
                                      (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int * 3)(*dims), out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            assert (out == 3.0).all(), "a refused call wrote something"
        return rc
    nanv = v.copy()
    nanv[3, 1] = np.nan
    assert mesh(v, np.array([[0, 1, 8]])) == -1 and mesh(nanv, t) == -1 and mesh(v, t[:0]) == -1
    assert mesh(v, t, dims=(2, 0, 2)) == -1 and mesh(v, t, spacing=(1, 0, 1)) == -1 and mesh(v, t, origin=(0, float("inf"), 0)) == -1
    assert mesh(v, t) == 0 and (out != 3.0).all()
