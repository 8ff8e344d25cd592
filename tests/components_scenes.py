"""The scenes of the connected-components tests (CPU twin and device): the smallest arrangements at which a union-find over the stencil
walk can go wrong.  scenes(pkg) yields (name, records, params, radius, expected number of bodies or None)."""
import numpy as np

from query_scenes import grid, params  # noqa: F401  (the box of 4 x 3 x 3.5 at h = 0.5; CS.params is what the test files call)
from support import records

F = np.float32


def rec_of(pkg, pos, ghost=None):
    pos = np.asarray(pos, F).reshape(-1, 3)
    return records(pkg, pos, np.zeros_like(pos), ghost=ghost)


def accepted(a, b, R):
    """neighbor_accept in fp32: r2 = fma(dz, dz, fma(dy, dy, dx * dx)) < R * R.  Exact here: the pairs differ along x only."""
    d = np.asarray(a, F) - np.asarray(b, F)
    assert d[1] == 0 and d[2] == 0
    return bool(F(d[0]) * F(d[0]) < F(R) * F(R))


def threshold_pair(a, R):
    """(inside, outside): the last fp32 x beyond a[0] that is accepted at R and the first that is not (same y, z)."""
    a = np.asarray(a, F)
    b = a.copy()
    b[0] = F(a[0] + F(R))
    assert abs(float(b[0])) > 1e-3                             # (the steps below are ulps of b)
    while accepted(a, b, R):
        b[0] = np.nextafter(b[0], F(np.inf))
    for _ in range(64):
        c = b.copy()
        c[0] = np.nextafter(b[0], F(-np.inf))
        if accepted(a, c, R):
            return c, b
        b = c
    raise AssertionError("no threshold within 64 ulps")


def crowd(pkg, sp, m, joined):
    """m records in one cell: inside a cube of half a cell (all within R = h of each other), or on a lattice of an eighth of a cell
    against R = 0.02 h (all apart).  Four far records keep them company."""
    lo, dims, cs = grid(pkg, sp)
    cell = np.array([3, 2, 4], F)
    rng = np.random.default_rng(m)
    if joined:
        pos = lo + (cell + F(0.25) + F(0.5) * rng.random((m, 3)).astype(F)) * cs
        R = float(sp.param_h)
    else:
        ijk = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(343)[:m]]
        pos = lo + (cell + F(0.0625) + F(0.125) * ijk.astype(F)) * cs
        R = float(F(0.02) * F(sp.param_h))
    far = lo + (np.array([[1, 1, 1], [6, 1, 1], [1, 5, 1], [1, 1, 7]], F) + F(0.5)) * cs
    return rec_of(pkg, np.concatenate([far, pos])), R, (5 if joined else m + 4)


def serpentine(pkg, sp, n=3000, cut=None):
    """A chain of n records with spacing 0.9 R (R = h) that snakes along x, row after row in y, layer after layer in z; rows are two
    steps apart.  cut: the index of a record to leave out (two bodies)."""
    lo, dims, cs = grid(pkg, sp)
    d = F(0.9) * F(sp.param_h)
    nx = int((dims[0] - 2) * cs / d)
    ymax = 2 * (int((dims[1] - 2) * cs / d) // 2 - 1)
    path = []
    x, y, z, dx, dy = 0, 0, 0, 1, 1
    while len(path) < n:
        for _ in range(nx):                                    # a row
            path.append((x, y, z))
            x += dx
        x -= dx
        dx = -dx
        if 0 <= y + 2 * dy <= ymax:                            # the connector to the next row, two steps on
            path.append((x, y + dy, z))
            y += 2 * dy
        else:                                                  # the end of a layer: up two steps, then back through the rows
            path.append((x, y, z + 1))
            z += 2
            dy = -dy
    assert (z + 2) * d < (dims[2] - 2) * cs
    pos = lo + cs + np.array(path[:n], F) * d
    if cut is not None:
        pos = np.delete(pos, cut, axis=0)
    return pos


def combs(pkg, sp):
    """Two interleaved combs in one plane: teeth along x, p = 1.5 R apart and alternately of body A (joined by a spine at the low end)
    and body B (spine at the high end), so both run through the same cells and never come within R of each other."""
    lo, dims, cs = grid(pkg, sp)
    R = F(0.3) * cs
    a, p = F(0.8) * R, F(1.5) * R
    teeth, length = 12, 40
    A, B = [], []
    for t in range(teeth):
        body = A if t % 2 == 0 else B
        first = 0 if t % 2 == 0 else 3                          # a tooth of B starts 3 a = 2.4 R beyond A's spine ...
        last = length - 3 if t % 2 == 0 else length             # ... and a tooth of A ends as far in front of B's
        body += [(i * a, t * p) for i in range(first, last)]
    for body, x in ((A, F(0)), (B, (length - 1) * a)):          # the spines: along y at the teeth's ends
        steps = int(np.ceil((teeth - 1) * p / a))
        body += [(x, j * ((teeth - 1) * p / steps)) for j in range(steps + 1)]
    pos = [(lo[0] + cs + x, lo[1] + cs + y, lo[2] + F(2.5) * cs) for x, y in A + B]
    return rec_of(pkg, pos), float(R)


def cloud(pkg, sp, seed):
    """500 - 5000 records uniform in the grid's box with a mean degree between 1 and 4: both sides of percolation."""
    lo, dims, cs = grid(pkg, sp)
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.integers(500, 5001))
    degree = float(rng.uniform(1.0, 4.0))
    ext = dims.astype(F) * cs
    R = float(F((degree * float(np.prod(ext)) / (n * 4.18879)) ** (1.0 / 3.0)))
    assert 0 < R <= 3 * cs
    pos = lo + rng.random((n, 3)).astype(F) * ext
    return rec_of(pkg, pos), R


def scenes(pkg):
    sp = params(pkg)
    lo, dims, cs = grid(pkg, sp)
    h = float(sp.param_h)
    at = lambda cell, frac: lo + (np.asarray(cell, F) + np.asarray(frac, F)) * cs      # noqa: E731
    yield "n = 0", rec_of(pkg, np.zeros((0, 3), F)), sp, h, 0
    yield "n = 1", rec_of(pkg, [at((2, 2, 2), (0.5, 0.5, 0.5))]), sp, h, 1
    yield "n = 2 apart", rec_of(pkg, [at((2, 2, 2), (0.5,) * 3), at((6, 5, 5), (0.5,) * 3)]), sp, h, 2
    yield "n = 2 joined", rec_of(pkg, [at((2, 2, 2), (0.5,) * 3), at((2, 2, 2), (0.75,) * 3)]), sp, h, 1
    # threshold pairs: in one cell (R = 0.4 h), in adjacent cells (R = h), at the outer ring of the stencil (R = 2 h, 3 h)
    for what, a, R in (("one cell", at((3, 3, 3), (0.05, 0.5, 0.5)), 0.4 * h), ("adjacent cells", at((3, 3, 3), (0.3, 0.5, 0.5)), h),
                       ("ring 2", at((2, 3, 3), (0.3, 0.5, 0.5)), 2.0 * h), ("ring 3", at((1, 3, 3), (0.3, 0.5, 0.5)), 3.0 * h)):
        R = float(F(R))
        inside, outside = threshold_pair(a, R)
        assert accepted(a, inside, R) and not accepted(a, outside, R)
        yield f"threshold {what}: below R", rec_of(pkg, [a, inside]), sp, R, 1
        yield f"threshold {what}: at R", rec_of(pkg, [a, outside]), sp, R, 2
    for m in (63, 64, 65, 200, 300):
        rec, R, bodies = crowd(pkg, sp, m, True)
        yield f"crowd {m} joined", rec, sp, R, bodies
        rec, R, bodies = crowd(pkg, sp, m, False)
        yield f"crowd {m} apart", rec, sp, R, bodies
    rec, R = combs(pkg, sp)
    yield "interleaved combs", rec, sp, R, 2
    # clamped cells: beyond the +x face, one clamped cell; 2 h apart (separate), and a third within R of the second (joined)
    hi = lo + dims.astype(F) * cs
    y, z = lo[1] + F(2.5) * cs, lo[2] + F(2.5) * cs
    out = [(hi[0] + F(5) * cs, y, z), (hi[0] + F(7) * cs, y, z), (hi[0] + F(7.5) * cs, y, z), (hi[0] - F(0.5) * cs, y, z)]
    yield "clamped cell", rec_of(pkg, out), sp, h, 3
    # a NaN and an infinite position among a blob: bodies of one, flagged
    blob = at((4, 3, 3), (0.5,) * 3) + F(0.2) * cs * np.random.default_rng(1).random((40, 3)).astype(F)
    bad = rec_of(pkg, blob)
    bad["pos"][7, 0] = np.nan
    bad["pos"][30, 2] = -np.inf
    yield "non-finite", bad, sp, h, 3
    # a ghost between two blobs, 0.8 R from each
    left = at((3, 3, 3), (0.5,) * 3)
    pts = [left, left + np.array([0.8 * h, 0, 0], F), left + np.array([1.6 * h, 0, 0], F), left - np.array([0.5 * h, 0, 0], F),
           left + np.array([2.1 * h, 0, 0], F)]
    yield "ghost bridge", rec_of(pkg, pts, ghost=np.array([0, 1, 0, 0, 0], np.int32)), sp, h, 1


def chain_scenes(pkg):
    """(name, positions in path order, params, radius, bodies): the serpentine chain, whole and cut, on a grid of h = 0.1."""
    sp = params(pkg, h=0.1)
    yield "chain", serpentine(pkg, sp), sp, float(sp.param_h), 1
    yield "chain cut", serpentine(pkg, sp, cut=1000), sp, float(sp.param_h), 2
