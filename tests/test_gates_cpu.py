"""Flow gates on the host: sph_gates_step_host, the twin of k_gates, against the numpy restatement of
tests/gates_ref.py, the hand cases of the definition, the two counting identities, and every refusal of a gate table.  No GPU."""
import numpy as np
import pytest

import gates_ref as GR
from gates_ref import check_books, mixed_gates
from support import records

F = np.float32


def recs(pkg, pos, vel=None, ghost=None):
    pos = np.asarray(pos, F).reshape(-1, 3)
    return records(pkg, pos, np.zeros_like(pos) if vel is None else np.asarray(vel, F).reshape(-1, 3), ghost)


def walk(pkg, rng, n, steps, step_size, half=1.0):
    """A random walk of n particles in the cube |x| < 1.5 half: the list of records after every step (the first one the start)."""
    pos = rng.uniform(-1.5 * half, 1.5 * half, (n, 3)).astype(F)
    out = [recs(pkg, pos, rng.normal(0, 1, (n, 3)))]
    for _ in range(steps):
        pos = (pos + rng.normal(0, step_size, (n, 3)).astype(F)).astype(F)
        pos = np.clip(pos, -1.5 * half, 1.5 * half).astype(F)
        out.append(recs(pkg, pos, rng.normal(0, 1, (n, 3))))
    return out


@pytest.mark.parametrize("K", [0, 1, 4])
def test_twin_equals_restatement(pkg, K):
    rng = np.random.default_rng(5 + K)
    states = walk(pkg, rng, 3000, 6, 0.25)
    for st in states:                                               # ghosts and non-finite positions take part in the input
        st["isGhost"][::97] = 1
    states[2]["pos"][5, 1] = np.nan
    states[3]["pos"][11, 0] = np.inf
    gates = mixed_gates(pkg, (0.1, -0.05, 0.2), 1.5)
    ref_gates = pkg.gate_array(gates).view(GR.GATE_DTYPE)
    total, books = None, None
    for a, b in zip(states[:-1], states[1:]):
        vals = None if K == 0 else rng.normal(1.0, 2.0, (len(a), K)).astype(F)
        if vals is not None:
            vals[::53, 0] = np.nan                                  # (a non-finite value adds 0)
        total = GR.add(total, GR.step(a, b, ref_gates, vals))
        books = pkg.gates_step_host(a, b, gates, vals, books)
    assert int((total["forward"] + total["backward"]).sum()) > 1000
    assert total["forward"][6] == 0 and total["backward"][6] == 0    # the empty gate
    check_books(books, total, f"K = {K}")
    assert (books["scalar"][:, K:] == 0).all()


def one(pkg, g, p0, p1, **kw):
    b = pkg.gates_step_host(recs(pkg, p0, **kw), recs(pkg, p1, **kw), [g])
    return int(b["forward"][0]), int(b["backward"][0])


def test_hand_cases(pkg):
    R, E = pkg.SPH_GATE_RECT, pkg.SPH_GATE_ELLIPSE
    g = pkg.gate(R, (0, 0, 0), (0, 0, 1), (1, 0, 0))                  # N = cross(z, x) = +y, half extents 1 x 1
    # landing exactly on the plane counts forward once, moving on does not count again
    assert one(pkg, g, (0.2, -0.5, 0.1), (0.2, 0.0, 0.1)) == (1, 0)
    assert one(pkg, g, (0.2, 0.0, 0.1), (0.2, 0.5, 0.1)) == (0, 0)
    assert one(pkg, g, (0.2, 0.0, 0.1), (0.2, -0.5, 0.1)) == (0, 1)   # from the plane backwards: s0 >= 0 && s1 < 0
    assert one(pkg, g, (0.2, 0.5, 0.1), (0.2, 0.25, 0.1)) == (0, 0)
    # exactly on the patch edge: excluded (strict <); just inside: counted
    assert one(pkg, g, (1.0, -0.5, 0.0), (1.0, 0.5, 0.0)) == (0, 0)
    assert one(pkg, g, (0.0, -0.5, 1.0), (0.0, 0.5, 1.0)) == (0, 0)
    assert one(pkg, g, (np.nextafter(F(1), F(0)), -0.5, 0.0), (np.nextafter(F(1), F(0)), 0.5, 0.0)) == (1, 0)
    # NaN at the entry or at the exit
    assert one(pkg, g, (np.nan, -0.5, 0.0), (0.0, 0.5, 0.0)) == (0, 0)
    assert one(pkg, g, (0.0, -0.5, 0.0), (0.0, np.nan, 0.0)) == (0, 0)
    # a ghost
    assert one(pkg, g, (0.0, -0.5, 0.0), (0.0, 0.5, 0.0), ghost=np.array([1])) == (0, 0)
    # the ellipse against the rectangle: the corner region belongs to the rectangle only
    e = pkg.gate(E, (0, 0, 0), (0, 0, 1), (1, 0, 0))
    assert one(pkg, g, (0.8, -0.5, 0.8), (0.8, 0.5, 0.8)) == (1, 0) and one(pkg, e, (0.8, -0.5, 0.8), (0.8, 0.5, 0.8)) == (0, 0)
    assert one(pkg, e, (0.6, -0.5, 0.6), (0.6, 0.5, 0.6)) == (1, 0)
    assert one(pkg, e, (0.0, -0.5, 1.0), (0.0, 0.5, 1.0)) == (0, 0)   # on the ellipse: fa^2 + fb^2 == 1
    # UNBOUNDED: the whole plane
    far = ((50.0, -0.5, -70.0), (50.0, 0.5, -70.0))
    assert one(pkg, g, *far) == (0, 0)
    assert one(pkg, pkg.gate(R, (0, 0, 0), (0, 0, 1), (1, 0, 0), unbounded=True), *far) == (1, 0)
    # swapping u and v flips forward and backward
    assert one(pkg, pkg.gate(R, (0, 0, 0), (1, 0, 0), (0, 0, 1)), (0.2, -0.5, 0.1), (0.2, 0.5, 0.1)) == (0, 1)
    # the signs of the sums: + forward, - backward, of the exit velocity and the values
    a, b = recs(pkg, [(0, -0.5, 0), (0.5, 0.5, 0)]), recs(pkg, [(0, 0.5, 0), (0.5, -0.5, 0)], vel=[(1, 2, 3), (10, 20, 30)])
    books = pkg.gates_step_host(a, b, [g], np.array([[0.5, 7.0], [0.25, np.inf]], F))
    assert books["vel"][0].tolist() == [-9.0, -18.0, -27.0] and books["scalar"][0].tolist() == [0.25, 7.0, 0.0, 0.0]


def test_unbounded_plane_identity(pkg):
    """forward - backward of a whole plane equals the change in the number of particles with s >= 0: exact by construction."""
    rng = np.random.default_rng(11)
    states = walk(pkg, rng, 4096, 32, 0.3)
    planes = [pkg.gate(pkg.SPH_GATE_RECT, (0.1, 0.2, -0.3), (0.6, 0.0, 0.8), (0.0, 2.0, 0.0), unbounded=True),
              pkg.gate(pkg.SPH_GATE_ELLIPSE, (0, 0, 0), (0, 0, 1), (1, 0, 0), unbounded=True)]
    ref = pkg.gate_array(planes).view(GR.GATE_DTYPE)
    books = None
    for a, b in zip(states[:-1], states[1:]):
        books = pkg.gates_step_host(a, b, planes, None, books)
    net = books["forward"].astype(np.int64) - books["backward"].astype(np.int64)
    for i in range(2):
        change = int(GR.above(ref[i], states[-1]).sum()) - int(GR.above(ref[i], states[0]).sum())
        assert int(books["forward"][i]) > 4096 and net[i] == change, (i, books[i], change)


def inside_box(rec, center, half):
    d = np.abs(rec["pos"][:, :3].astype(np.float64) - np.asarray(center, np.float64))
    return (d < np.asarray(half, np.float64)).all(axis=1)


def test_control_volume_identity(pkg):
    """Net outflow through gate_box equals the loss of particles inside.  Not a theorem (a crossing within a rounding of a box edge can
    be booked twice or not at all), so the seed is one for which the twin itself satisfies the identity; the walk's small steps keep
    such crossings rare."""
    rng = np.random.default_rng(2)
    center, half = (0.05, -0.1, 0.15), (0.7, 0.6, 0.8)
    states = walk(pkg, rng, 4096, 32, 0.05)
    box = pkg.gate_box(center, half)
    assert len(box) == 6
    books = None
    for a, b in zip(states[:-1], states[1:]):
        books = pkg.gates_step_host(a, b, box, None, books)
    out = int(books["forward"].astype(np.int64).sum() - books["backward"].astype(np.int64).sum())
    crossings = int(books["forward"].sum() + books["backward"].sum())
    loss = int(inside_box(states[0], center, half).sum()) - int(inside_box(states[-1], center, half).sum())
    assert crossings > 1000 and out == loss, (out, loss, crossings)
    # outward normals: a particle leaving through each face is forward on that face alone
    for f, (axis, sign) in enumerate([(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]):
        p0, p1 = np.array(center, F), np.array(center, F)
        p1[axis] += sign * 1.5 * half[axis]
        b = pkg.gates_step_host(recs(pkg, p0), recs(pkg, p1), box)
        assert b["forward"].tolist() == [1 if i == f else 0 for i in range(6)] and not b["backward"].any(), f


def test_discharge(pkg):
    sp = pkg.default_params(param_mass=2.0, param_restDensity=1000.0)
    rows = np.zeros(2, pkg.GATE_BOOKS_DTYPE)
    rows["forward"], rows["backward"] = (30, 5), (10, 5)
    assert pkg.gate_discharge(rows, 0.5, sp).tolist() == [20 * 2.0 / 1000.0 / 0.5, 0.0]


def refused(pkg, gates, **kw):
    L = pkg.load_library()
    arr = pkg.gate_array(gates)
    books = np.zeros(8, pkg.GATE_BOOKS_DTYPE)
    count = kw.get("count", len(arr))
    rc = L.sph_gates_step_host(None, None, 0, arr.ctypes.data if len(arr) and not kw.get("null") else None, count, None, 0, books.ctypes.data)
    return rc, L.sph_last_error().decode()


def test_refusals_of_a_gate_table(pkg):
    """What sph_gates_set refuses about the table itself, through the twin (the same check; the engine's own refusals need a device)."""
    R = pkg.SPH_GATE_RECT
    ok = pkg.gate(R, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert refused(pkg, [ok])[0] == 0
    assert refused(pkg, [ok] * 9)[0] == -1                                        # a count above 8
    assert refused(pkg, [ok], null=True)[0] == -1                                 # a null table with a count > 0
    bad = pkg.gate(2, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert refused(pkg, [ok, bad]) == (-1, "gate 1: unknown shape 2")
    bad = pkg.gate(R, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    bad.flags = 2
    assert refused(pkg, [bad])[0] == -1 and "flag" in refused(pkg, [bad])[1]
    for field in ("center", "u", "v"):
        for value in (np.nan, np.inf):
            bad = pkg.gate(R, (0, 0, 0), (1, 0, 0), (0, 1, 0))
            getattr(bad, field)[1] = value
            assert refused(pkg, [bad]) == (-1, "gate 0: a field is not finite"), field
    assert "zero length" in refused(pkg, [pkg.gate(R, (0, 0, 0), (0, 0, 0), (0, 1, 0))])[1]
    assert "zero length" in refused(pkg, [pkg.gate(R, (0, 0, 0), (1, 0, 0), (0, 0, 0))])[1]
    assert "orthogonal" in refused(pkg, [pkg.gate(R, (0, 0, 0), (1, 0, 0), (2e-4, 1, 0))])[1]      # |u.v| > 1e-4 |u| |v|
    assert refused(pkg, [pkg.gate(R, (0, 0, 0), (1, 0, 0), (0.5e-4, 1, 0))])[0] == 0
    assert refused(pkg, [pkg.gate(R, (0, 0, 0), (1e-3, 0, 0), (0, 1e3, 0))])[0] == 0               # any lengths


def test_layouts_and_box(pkg, tmp_path):
    from support import c_layout
    size, offsets, extra = c_layout("SphGate", pkg.SphGate, ['printf("%zu %d %d\\n", sizeof(SphGateBooks), SPH_MAX_GATES, SPH_MAX_GATE_HISTORY);'], tmp_path)
    assert size == 64 and offsets == [(n, getattr(pkg.SphGate, n).offset) for n, _ in pkg.SphGate._fields_]
    assert extra == [f"72 {pkg.SPH_MAX_GATES} {pkg.SPH_MAX_GATE_HISTORY}"]
    box = pkg.gate_array(pkg.gate_box((1, 2, 3), (0.5, 0.25, 2.0))).view(GR.GATE_DTYPE)
    want = np.array(GR.gate_box((1, 2, 3), (0.5, 0.25, 2.0)))
    assert box.tobytes() == want.tobytes()
    normals = np.array([GR.normal(g) for g in box])
    assert (np.sign(normals) == np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]])).all()
