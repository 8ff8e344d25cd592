"""Restatement of the connected components (include/sph_abi.h "connected components") in numpy and plain Python: a union-find over the
undirected pairs of neighbors_ref.brute_force(..., half=True), the canonical names (root = smallest id, bodies numbered in ascending
order of it) and the table with Python-integer position sums.  Like the brute force it knows nothing of stencils or rounding in the
accept test: it agrees with the engine where `margin` (the smallest |r^2 - R^2| / R^2 over all pairs) is well above rounding."""
import numpy as np

import neighbors_ref as NR

F = np.float32


def fixed_point(pkg, pos, sp):
    """(n, 3) Python-exact int64 of llrint(clamp(((double)x - (double)gridMin) * S, -2^36, 2^36)), S = 65536.0 / (double)cellSize."""
    g = pkg.compute_grid_extents(sp)
    gmin = np.array(list(g.gridMin), F).astype(np.float64)
    S = np.float64(65536.0) / np.float64(F(g.cellSize))
    x = np.asarray(pos, F)[:, :3].astype(np.float64)
    d = (np.where(np.isfinite(x), x, 0.0) - gmin) * S                                 # (a non-finite record has no sums)
    return np.rint(np.clip(d, -2.0 ** 36, 2.0 ** 36)).astype(np.int64)                # (rint: to nearest even)


def union_find(n, pairs):
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64)                             # the smaller root wins: a root is its tree's smallest id


def components(pkg, rec, sp, radius, fluid_only=False):
    """(labels int32[n], roots int32[n], table dict of arrays with Python-integer sumQ, margin) of the records `rec`."""
    pos = rec["pos"]
    n = len(rec)
    off, idx, margin = NR.brute_force(pkg, pos, sp, radius, half=True)
    recv = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    send = idx.astype(np.int64)
    part = np.ones(n, bool) if not fluid_only else (rec["isGhost"] == 0)
    keep = part[recv] & part[send]
    root = union_find(n, zip(recv[keep], send[keep]))
    roots = np.where(part, root, -1).astype(np.int32)
    heads = np.flatnonzero(part & (root == np.arange(n)))                              # ascending: the numbering
    number = np.full(n, -1, np.int64)
    number[heads] = np.arange(len(heads))
    labels = np.where(part, number[np.where(part, root, 0)], -1).astype(np.int32)
    q = fixed_point(pkg, pos, sp) if n else np.zeros((0, 3), np.int64)
    finite = np.isfinite(np.asarray(pos, F)[:, :3]).all(axis=1)
    C = len(heads)
    table = dict(root=heads.astype(np.uint32), count=np.zeros(C, np.uint32), bbMin=np.zeros((C, 3), F), bbMax=np.zeros((C, 3), F),
                 sumQ=[[0, 0, 0] for _ in range(C)], flags=np.zeros(C, np.uint32))
    members = [[] for _ in range(C)]
    for i in np.flatnonzero(part):
        members[labels[i]].append(int(i))
    for c, m in enumerate(members):
        table["count"][c] = len(m)
        if not finite[m].all():
            assert len(m) == 1, "a non-finite record is accepted by nobody"
            table["flags"][c] = pkg.SPH_COMPONENT_NONFINITE
            continue
        p = np.asarray(pos, F)[m, :3]
        table["bbMin"][c], table["bbMax"][c] = p.min(axis=0), p.max(axis=0)
        table["sumQ"][c] = [sum(int(v) for v in q[m, a]) for a in range(3)]
    return labels, roots, table, margin


def assert_table(got, want, what=""):
    """An engine table (COMPONENT_DTYPE) against the restatement's."""
    assert len(got) == len(want["root"]), f"{what}: {len(got)} bodies, expected {len(want['root'])}"
    assert np.array_equal(got["root"], want["root"]) and np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["flags"], want["flags"]) and not got["pad"].any(), what
    assert np.array_equal(got["bbMin"], want["bbMin"]) and np.array_equal(got["bbMax"], want["bbMax"]), what
    assert [[int(v) for v in row] for row in got["sumQ"]] == want["sumQ"], what


def info_of(labels, roots, table):
    """What SphComponentInfo must say about (labels, roots, table), except radius, stencil, flags and rounds."""
    cnt = table["count"].astype(np.int64)
    big = int(np.argmax(cnt)) if len(cnt) else 0                                      # (argmax: the first of equals, i.e. the smaller root)
    return dict(rows=len(labels), numComponents=len(cnt), numExcluded=int((labels < 0).sum()), largestCount=int(cnt[big]) if len(cnt) else 0,
                largestRoot=int(table["root"][big]) if len(cnt) else 0, numSingletons=int((cnt == 1).sum()))
