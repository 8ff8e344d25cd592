"""Iso-surface meshes without a GPU: the contract of DESIGN.md section 3b restated in numpy (tests/surface_ref.py) is a closed,
oriented 2-manifold of the right topology and converges to the true surface; the C-ABI and Python mirror expose the new entry points.

Measured on the sphere f = R - |x - c|, R = 12 (isotropic spacing 1) and R = 12 * 0.9 (spacing 0.7, 0.9, 1.1):
  isotropic:   volume / (4/3 pi R^3) = 0.99653, area / (4 pi R^2) = 0.9982, largest normal error 0.19 deg
  anisotropic: volume / (4/3 pi R^3) = 0.99641, area / (4 pi R^2) = 0.9982, largest normal error 0.23 deg
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import surface_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _kuhn_euler(inside):
    """Euler characteristic of the full subcomplex of the lattice's Kuhn complex on the inside points: a k-simplex is a base point
    and a strictly nested chain of k non-empty corner sets d1 < d2 < ... (each vertex base + offset(d))."""
    nz, ny, nx = inside.shape
    pts = np.argwhere(inside)
    chi = 0
    chains = [c for k in range(1, 4) for c in itertools.combinations(range(1, 8), k) if all(c[q] & c[q + 1] == c[q] for q in range(k - 1))]
    chi += len(pts)
    for l, j, i in pts:
        for c in chains:
            ok = True
            for d in c:
                ll, jj, ii = l + ((d >> 2) & 1), j + ((d >> 1) & 1), i + (d & 1)
                if ll >= nz or jj >= ny or ii >= nx or not inside[ll, jj, ii]:
                    ok = False
                    break
            if ok:
                chi += (-1) ** len(c)
    return chi


def test_all_256_patterns_of_one_cube():
    """Every inside pattern of one cube, the rest of a 4^3 lattice outside: closed and oriented, and the surface's Euler
    characteristic is twice the inside region's (computed independently on the Kuhn complex).  Every component is a sphere
    (chi = 2) except for one pattern: corners 1..6 inside, 0 and 7 outside, where the six inside corners are joined by Kuhn
    edges into a ring (1-3-2-6-4-5) and the surface is one torus (chi = 0)."""
    tori = []
    for pat in range(256):
        f = np.zeros((4, 4, 4), F)
        for c in range(8):
            if (pat >> c) & 1:
                f[1 + ((c >> 2) & 1), 1 + ((c >> 1) & 1), 1 + (c & 1)] = 1.0
        pos, nrm, tris = sr.extract(f, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.5)
        if pat == 0:
            assert len(tris) == 0 and len(pos) == 0
            continue
        assert sr.closed_oriented(tris), pat
        assert len(np.unique(tris)) == len(pos), pat                          # every vertex is used
        chi = sr.euler_per_component(tris)
        assert sum(chi) == 2 * _kuhn_euler(f >= 0.5), pat
        if chi != [2] * len(chi):
            tori.append((pat, chi))
        assert sr.enclosed_volume(pos, tris) > 0, pat                         # outward winding
    assert tori == [(0b01111110, [0])]


def test_random_fields_are_closed_and_oriented():
    rng = np.random.default_rng(1)
    for it in range(200):
        f = rng.random((7, 9, 11)).astype(F)
        f[rng.random(f.shape) < 0.15] = F(0.5)                               # exactly iso: inside, zero-area triangles kept
        f[rng.random(f.shape) < 0.1] = F(0.25)
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 0, 0, 0, 0, 0, 0
        pos, nrm, tris = sr.extract(f, (-1.5, 0.25, 3.0), (0.5, 0.75, 1.25), 0.5)
        assert len(tris) > 0
        assert sr.closed_oriented(tris), it
        assert tris.max() < len(pos)
        assert sum(sr.euler_per_component(tris)) == 2 * _kuhn_euler(f >= F(0.5)), it


def test_open_only_along_the_outer_layer():
    rng = np.random.default_rng(2)
    f = rng.random((6, 7, 8)).astype(F)
    pos, nrm, tris = sr.extract(f, (0, 0, 0), (1, 1, 1), 0.5)
    b = sr.boundary_edges(tris)
    assert len(b) > 0
    p = pos[b.reshape(-1)]
    hi = np.array([7, 6, 5], F)
    on_layer = ((p <= 1.0) | (p >= hi - 1.0)).any(axis=1)                   # an end on an outer-layer edge or face
    assert on_layer.all()


def _sphere(R, spacing, centre_shift=(0.31, -0.17, 0.23)):
    s = np.array(spacing, np.float64)
    n = (np.ceil(2 * (R + 3) / s)).astype(int) + 1
    origin = -(n - 1) / 2.0 * s
    xs, ys, zs = sr.lattice_axes(origin, s, n)
    c = np.array(centre_shift) * s
    Z, Y, X = np.meshgrid(zs.astype(np.float64), ys.astype(np.float64), xs.astype(np.float64), indexing="ij")
    f = (R - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(F)
    return f, origin, s, c


@pytest.mark.parametrize("spacing,R", [((1.0, 1.0, 1.0), 12.0), ((0.7, 0.9, 1.1), 12.0 * 0.9)])
def test_sphere_volume_area_normals(spacing, R):
    f, origin, s, c = _sphere(R, spacing)
    pos, nrm, tris = sr.extract(f, origin, s, 0.0)
    assert sr.closed_oriented(tris)
    assert sr.euler_per_component(tris) == [2]
    vol = sr.enclosed_volume(pos, tris) / (4.0 / 3.0 * np.pi * R ** 3)
    ar = sr.area(pos, tris) / (4.0 * np.pi * R ** 2)
    d = pos.astype(np.float64) - c
    want = d / np.linalg.norm(d, axis=1)[:, None]
    ang = np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", nrm.astype(np.float64), want), -1, 1)))
    print(f"spacing {spacing}: volume ratio {vol:.5f}, area ratio {ar:.4f}, largest normal error {ang.max():.2f} deg")
    assert abs(vol - 1.0) < 0.01
    assert abs(ar - 1.0) < 0.05
    assert ang.max() < 5.0


def test_two_spheres_and_a_torus():
    n = 48
    xs = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    Z, Y, X = np.meshgrid(xs, xs, xs, indexing="ij")
    two = np.maximum(7 - np.sqrt((X - 10) ** 2 + Y ** 2 + Z ** 2), 6 - np.sqrt((X + 11) ** 2 + (Y - 2) ** 2 + Z ** 2)).astype(F)
    pos, nrm, tris = sr.extract(two, (0, 0, 0), (1, 1, 1), 0.0)
    assert sr.closed_oriented(tris)
    assert sr.euler(tris) == 4 and sr.euler_per_component(tris) == [2, 2]
    torus = (5 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 14) ** 2 + Z ** 2)).astype(F)
    pos, nrm, tris = sr.extract(torus, (0, 0, 0), (1, 1, 1), 0.0)
    assert sr.closed_oriented(tris)
    assert sr.euler(tris) == 0 and sr.euler_per_component(tris) == [0]
    assert sr.enclosed_volume(pos, tris) == pytest.approx(2 * np.pi ** 2 * 14 * 25, rel=0.02)


def test_surface_entry_points_and_layout(pkg):
    """The three entry points are exported and declared, the vertex record is 24 bytes, and each call refuses a null engine."""
    import re
    L = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "sph_abi.h")).read()
    for sym in ("sph_extract_surface", "sph_extract_surface_volume", "sph_surface_download"):
        assert sym in pkg.ABI_SYMBOLS and hasattr(L, sym) and re.search(r"\bint " + sym + r"\(", src)
    assert pkg.SURFACE_VERTEX_DTYPE.itemsize == 24
    assert pkg.SURFACE_VERTEX_DTYPE.fields["pos"][1] == 0 and pkg.SURFACE_VERTEX_DTYPE.fields["normal"][1] == 12
    assert C.sizeof(pkg.SphSurface) == 24 and pkg.SphSurface.vertices.offset == 8 and pkg.SphSurface.triangles.offset == 16
    assert re.search(r"#define SPH_ABI_VERSION 4\b", src)
    f3, dims, s = pkg.engine._f3, (C.c_int * 3)(4, 4, 4), pkg.SphSurface()
    buf = np.zeros(64, F)
    assert L.sph_extract_surface(None, f3((0, 0, 0)), f3((1, 1, 1)), dims, pkg.SPH_FIELD_FRACTION, 0.5, C.byref(s)) == -1
    assert L.sph_extract_surface_volume(None, buf.ctypes.data_as(C.c_void_p), f3((0, 0, 0)), f3((1, 1, 1)), dims, 0.5, C.byref(s)) == -1
    v = np.zeros(4, pkg.SURFACE_VERTEX_DTYPE)
    t = np.zeros((4, 3), np.uint32)
    assert L.sph_surface_download(None, v.ctypes.data_as(C.c_void_p), 4, t.ctypes.data_as(C.c_void_p), 4) == -1


def test_write_ply_round_trip(pkg, tmp_path):
    f, origin, s, c = _sphere(4.0, (1.0, 1.0, 1.0))
    pos, nrm, tris = sr.extract(f, origin, s, 0.0)
    v = np.zeros(len(pos), pkg.SURFACE_VERTEX_DTYPE)
    v["pos"], v["normal"] = pos, nrm
    path = tmp_path / "s.ply"
    pkg.write_ply(str(path), v, tris)
    data = path.read_bytes()
    head, body = data.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    assert f"element vertex {len(v)}".encode() in head and f"element face {len(tris)}".encode() in head
    assert len(body) == 24 * len(v) + 13 * len(tris)
    assert body[: 24 * len(v)] == v.tobytes()
    faces = np.frombuffer(body[24 * len(v):], np.dtype([("n", "u1"), ("idx", "<u4", (3,))]))
    assert (faces["n"] == 3).all() and np.array_equal(faces["idx"], tris)
