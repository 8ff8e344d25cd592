"""Independent numpy restatement of the iso-surface contract, for tests/test_surface_cpu.py and
tests/test_gpu_surface.py.  It generates its own tet table from the definition and never reads the library's; every fp32 step
is a separate numpy float32 operation (numpy does not fuse a multiply and an add), so the GPU result must match it bit for bit.

  extract(f, origin, spacing, iso) -> (pos[V, 3], normal[V, 3], tris[T, 3])      f has shape (nz, ny, nx), x fastest
  mesh checks: closed_oriented, components, euler, enclosed_volume, area
"""
import numpy as np

F = np.float32
AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # xyz, xzy, yxz, yzx, zxy, zyx


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64)


def tet_chain(order):
    a, b, _ = order
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def make_table():
    """table[tet][case] = list of triangles; a triangle is 3 lattice edges (start corner, direction d).  Case bit k: chain corner
    m_k inside."""
    table = []
    for order in AXIS_ORDERS:
        m = tet_chain(order)

        def edge(k, l):
            k, l = min(k, l), max(k, l)
            return (m[k], m[l] ^ m[k])

        def mid(e):                                # the t = 1/2 point of an edge, in cube-corner units
            return corner_offset(e[0]) + 0.5 * corner_offset(e[1])

        row = []
        for case in range(16):
            ins = [k for k in range(4) if (case >> k) & 1]
            outs = [k for k in range(4) if not (case >> k) & 1]
            if len(ins) == 1:
                tris = [[edge(ins[0], r) for r in outs]]
            elif len(outs) == 1:
                tris = [[edge(outs[0], r) for r in ins]]
            elif len(ins) == 2:
                q = [edge(ins[0], outs[0]), edge(ins[0], outs[1]), edge(ins[1], outs[1]), edge(ins[1], outs[0])]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                tris = []
            if tris:
                want = np.mean([corner_offset(m[k]) for k in outs], axis=0) - np.mean([corner_offset(m[k]) for k in ins], axis=0)
            out = []
            for a, b, c in tris:
                nrm = np.cross(mid(b) - mid(a), mid(c) - mid(a))
                dot = float(nrm @ want)
                assert dot != 0.0
                out.append((a, b, c) if dot > 0 else (a, c, b))
            row.append(out)
        table.append(row)
    return table


TABLE = make_table()


def lattice_axes(origin, spacing, dims):
    """Point coordinates per axis: origin + (float)i * spacing, an fp32 multiply and then an add."""
    return [(F(origin[a]) + np.arange(dims[a]).astype(F) * F(spacing[a])).astype(F) for a in range(3)]


def _gradient(f, coords, axis):
    """g = (f[+] - f[-]) / (x[+] - x[-]) along array axis `axis` (2: x, 1: y, 0: z); one-sided on the first and last point."""
    n = f.shape[axis]
    idx = np.arange(n)
    hi, lo = np.minimum(idx + 1, n - 1), np.maximum(idx - 1, 0)
    df = (np.take(f, hi, axis=axis) - np.take(f, lo, axis=axis)).astype(F)
    dx = (coords[hi] - coords[lo]).astype(F)
    shape = [1, 1, 1]
    shape[axis] = n
    with np.errstate(all="ignore"):
        return (df / dx.reshape(shape)).astype(F)


def extract(f, origin, spacing, iso):
    f = np.ascontiguousarray(f, F)
    nz, ny, nx = f.shape
    assert min(nx, ny, nz) >= 2
    iso = F(iso)
    with np.errstate(invalid="ignore"):
        inside = f >= iso
    xs, ys, zs = lattice_axes(origin, spacing, (nx, ny, nz))
    # crossed[l, j, i, d - 1]: the edge from (i, j, l) in direction d, both ends in the lattice, inside at one end only
    crossed = np.zeros((nz, ny, nx, 7), bool)
    for d in range(1, 8):
        ox, oy, oz = d & 1, (d >> 1) & 1, (d >> 2) & 1
        a = inside[: nz - oz, : ny - oy, : nx - ox]
        b = inside[oz:, oy:, ox:]
        crossed[: nz - oz, : ny - oy, : nx - ox, d - 1] = a != b
    flat = crossed.reshape(-1)
    vid = np.full(flat.shape, -1, np.int64)
    sel = np.nonzero(flat)[0]                       # point-major, then d: the vertex order
    vid[sel] = np.arange(len(sel))
    p = sel // 7
    d = sel % 7 + 1
    i, j, l = p % nx, (p // nx) % ny, p // (nx * ny)
    ib, jb, lb = i + (d & 1), j + ((d >> 1) & 1), l + ((d >> 2) & 1)
    fa, fb = f[l, j, i], f[lb, jb, ib]
    with np.errstate(all="ignore"):
        t = ((iso - fa).astype(F) / (fb - fa).astype(F)).astype(F)
        pos = np.empty((len(sel), 3), F)
        for ax, (c, ia, ibb) in enumerate(((xs, i, ib), (ys, j, jb), (zs, l, lb))):
            pa, pb = c[ia], c[ibb]
            pos[:, ax] = pa + (t * (pb - pa).astype(F)).astype(F)
        g = [_gradient(f, xs, 2), _gradient(f, ys, 1), _gradient(f, zs, 0)]
        n = np.empty((len(sel), 3), F)
        for ax in range(3):
            ga, gb = g[ax][l, j, i], g[ax][lb, jb, ib]
            n[:, ax] = -(ga + (t * (gb - ga).astype(F)).astype(F))
        ss = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(F) + (n[:, 2] * n[:, 2]).astype(F)).astype(F)
        r = np.sqrt(ss).astype(F)
        zero = ss == F(0)
        normal = np.where(zero[:, None], F(0), n / np.where(zero, F(1), r)[:, None]).astype(F)
    tris = _triangles(inside, vid, nx, ny, nz)
    return pos, normal, tris


def _triangles(inside, vid, nx, ny, nz, chunk=1 << 18):
    tc = np.zeros((6, 16, 2, 3), np.int64)       # start corner
    td = np.ones((6, 16, 2, 3), np.int64)        # direction
    tn = np.zeros((6, 16), np.int64)
    for tet in range(6):
        for case in range(16):
            tn[tet, case] = len(TABLE[tet][case])
            for s, tri in enumerate(TABLE[tet][case]):
                for v, (c, d) in enumerate(tri):
                    tc[tet, case, s, v], td[tet, case, s, v] = c, d
    corners = [inside[(c >> 2) & 1: nz - 1 + ((c >> 2) & 1), (c >> 1) & 1: ny - 1 + ((c >> 1) & 1), c & 1: nx - 1 + (c & 1)].reshape(-1)
               for c in range(8)]
    nin = sum(c.astype(np.int8) for c in corners)
    mixed = np.nonzero((nin > 0) & (nin < 8))[0]                              # (cubes with all corners alike have no triangles)
    corners = [c[mixed] for c in corners]
    ci, cj, cl = mixed % (nx - 1), (mixed // (nx - 1)) % (ny - 1), mixed // ((nx - 1) * (ny - 1))
    cube_pt = ((cl * ny + cj) * nx + ci).astype(np.int64)
    coff = np.array([(c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny for c in range(8)], np.int64)
    out = []
    for s0 in range(0, len(cube_pt), chunk):
        sl = slice(s0, s0 + chunk)
        cases = []
        for order in AXIS_ORDERS:
            m = tet_chain(order)
            cases.append(sum(corners[m[k]][sl].astype(np.int64) << k for k in range(4)))
        cs = np.stack(cases, axis=1)                                          # (cubes, 6)
        tet = np.arange(6)[None, :]
        valid = np.arange(2)[None, None, :] < tn[tet, cs][:, :, None]       # (cubes, 6, 2)
        c = tc[tet, cs]                                                       # (cubes, 6, 2, 3)
        d = td[tet, cs]
        q = cube_pt[sl][:, None, None, None] + coff[c]
        idx = vid[q * 7 + d - 1]
        tri = idx[valid]
        assert (tri >= 0).all()
        out.append(tri)
    return np.concatenate(out).astype(np.uint32) if out else np.zeros((0, 3), np.uint32)


# ---- mesh checks ---------------------------------------------------------------------------------------------------------
def closed_oriented(tris):
    """Every directed edge in at most one triangle and its reverse in exactly one: every undirected edge in exactly two triangles,
    consistently oriented."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return True
    nv = int(t.max()) + 1
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    fwd = a * nv + b
    if len(np.unique(fwd)) != len(fwd):
        return False
    rev = np.sort(b * nv + a)
    return bool(np.array_equal(np.sort(fwd), rev))


def boundary_edges(tris):
    """Directed edges whose reverse is in no triangle."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return np.zeros((0, 2), np.int64)
    nv = int(t.max()) + 1
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    open_ = ~np.isin(b * nv + a, a * nv + b)
    return np.stack([a[open_], b[open_]], axis=1)


def components(tris):
    """Label of every triangle: the connected components of the mesh (through shared vertices)."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return np.zeros(0, np.int64)
    lab = np.arange(int(t.max()) + 1)
    while True:
        m = np.minimum(np.minimum(lab[t[:, 0]], lab[t[:, 1]]), lab[t[:, 2]])
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, t[:, k], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return lab[t[:, 0]]


def euler(tris):
    """V - E + F of a mesh (V: vertices referenced)."""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return 0
    e = np.sort(np.stack([np.concatenate([t[:, 0], t[:, 1], t[:, 2]]), np.concatenate([t[:, 1], t[:, 2], t[:, 0]])], axis=1), axis=1)
    return len(np.unique(t)) - len(np.unique(e, axis=0)) + len(t)


def euler_per_component(tris):
    lab = components(tris)
    t = np.asarray(tris)
    return sorted(euler(t[lab == c]) for c in np.unique(lab))


def enclosed_volume(pos, tris):
    """Divergence theorem, float64: sum of a . (b x c) / 6."""
    p = np.asarray(pos, np.float64)
    t = np.asarray(tris, np.int64)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(pos, tris):
    p = np.asarray(pos, np.float64)
    t = np.asarray(tris, np.int64)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
