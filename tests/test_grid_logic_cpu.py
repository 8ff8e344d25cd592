"""The counting sort's lane logic, restated wave by wave in Python and run over the scenes of grid_scenes.py (no GPU).

emulate_bin restates k_bin (csrc/sph_kernels.h, the lines from `const unsigned long long upto` to the binKey store): the head ballot,
startLane / endLane, one add per head, the slot handed to each lane.  The order in which the heads' atomic adds arrive is free on the
device; here they are applied in several seeded orders.  emulate_rank restates k_rank (the lines from `const uint32_t nLive` to the
order[] store): the shuffle loop for mWave <= 64, the every-lane branch above that, the gathers in front of d0 and behind d0 + 64, and
the inactive lanes of the last wave, which stay for the shuffles.  The scan between them is a plain cumulative sum here; its seams are
the GPU tests' subject.

For every scene and arrival order: the counts are oracle.build_grid's, the slots inside a cell are a permutation, and the final order
is the stable sort by (cell, id), oracle.build_grid's `order`.  The same file asserts that the scenes reach what they claim."""
import numpy as np
import pytest

from conftest import to_oracle_params
import grid_scenes as GS

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
DEAD = 0xFFFFFFFF
ARRIVAL_SEEDS = (None, 1, 2)              # None: program order


def _clz64(x):
    return 64 - x.bit_length()


def _ffs64(x):
    return (x & -x).bit_length()           # 1-based index of the lowest set bit, 0 for 0


def emulate_bin(cells, num_cells, arrival_seed):
    """k_bin over particle cells in state order: (binKey cell, binKey slot, histogram)."""
    n = len(cells)
    heads_out = []                                                     # (cell, amount, wave, lane) of every returning atomic
    per_wave = []
    for w0 in range(0, -(-n // GS.BLOCK) * GS.BLOCK, GS.WAVE):          # every wave of every launched block
        cell = [int(cells[w0 + l]) if w0 + l < n else DEAD for l in range(GS.WAVE)]      # `cell` of the lanes (0xFFFFFFFF: beyond n)
        head = [l == 0 or cell[l] != cell[l - 1] for l in range(GS.WAVE)]                 # prev = __shfl_up(cell, 1); lane 0 is a head
        heads = sum(1 << l for l in range(GS.WAVE) if head[l])                            # __ballot(head)
        lanes = []
        for l in range(GS.WAVE):
            upto = ((2 << l) - 1) & M64                                                   # bits 0..lane
            start_lane = 63 - _clz64(heads & upto)
            above = heads & ~upto & M64
            end_lane = _ffs64(above) - 1 if above else 64
            if head[l] and cell[l] != DEAD:
                heads_out.append((cell[l], end_lane - l, w0, l))
            lanes.append(start_lane)
        per_wave.append((w0, cell, lanes))
    order = np.arange(len(heads_out)) if arrival_seed is None else np.random.default_rng(arrival_seed).permutation(len(heads_out))
    count = np.zeros(num_cells, np.int64)
    base = {}
    for a in order:                                                    # base = atomicAdd(&cellCount[cell], endLane - lane)
        c, amount, w0, l = heads_out[a]
        base[(w0, l)] = int(count[c])
        count[c] += amount
    key_cell, key_slot = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for w0, cell, lanes in per_wave:
        for l in range(GS.WAVE):
            if w0 + l < n:                                             # if (inRange) binKey[i] = (cell, base of startLane + lane - startLane)
                key_cell[w0 + l] = cell[l]
                key_slot[w0 + l] = (base.get((w0, lanes[l]), 0) + l - lanes[l]) & M32
    return key_cell, key_slot, count


def emulate_scatter(key_cell, key_slot, cell_start):
    """k_scatter: tmp[cellStart[cell] + slot] = (source index, cell).  A slot written twice or left out fails here."""
    n = len(key_cell)
    tmp = np.full((n, 2), -1, np.int64)
    for i in range(n):
        d = cell_start[key_cell[i]] + key_slot[i]
        assert 0 <= d < n and tmp[d, 0] == -1, f"slot {d} of source {i}"
        tmp[d] = (i, key_cell[i])
    return tmp


def emulate_rank(tmp, cell_start, ids, num_cells):
    """k_rank<false, true>: order[s + rank] = source index, ranks by ascending id inside a cell."""
    n = len(tmp)
    n_live = int(cell_start[num_cells])
    id_of_slot = ids[tmp[:, 0]]                                        # fbits(vel[tmp[q].x].w) of the gathers
    order = np.full(n, -1, np.int64)
    for d0 in range(0, -(-n // GS.BLOCK) * GS.BLOCK, GS.WAVE):
        if (d0 // GS.BLOCK) * GS.BLOCK >= n_live:                      # whole block beyond the live particles
            continue
        act = [d0 + l < n and d0 + l < n_live for l in range(GS.WAVE)]
        src = [int(tmp[d0 + l, 0]) if act[l] else 0 for l in range(GS.WAVE)]
        c = [int(tmp[d0 + l, 1]) if act[l] else 0 for l in range(GS.WAVE)]
        s = [int(cell_start[c[l]]) if act[l] else 0 for l in range(GS.WAVE)]
        e = [int(cell_start[c[l] + 1]) if act[l] else 0 for l in range(GS.WAVE)]
        my = [int(ids[src[l]]) if act[l] else 0 for l in range(GS.WAVE)]                  # V stays zero in an inactive lane
        m = [(e[l] - s[l]) & M32 for l in range(GS.WAVE)]
        m_wave = max(m)
        rank = [0] * GS.WAVE
        if m_wave > 1:
            for l in range(GS.WAVE):
                if m_wave <= 64:
                    for j in range(m_wave):
                        lane_src = (s[l] + j - d0) & M32                                  # a member in front of the wave wraps
                        idq = my[lane_src & 63]
                        rank[l] += 1 if (j < m[l] and lane_src < 64 and idq < my[l]) else 0
                else:
                    for L in range(GS.WAVE):
                        q = d0 + L
                        rank[l] += 1 if (s[l] <= q < e[l] and my[L] < my[l]) else 0
                rank[l] += int((id_of_slot[s[l]:min(e[l], d0)] < my[l]).sum())            # members in front of the wave's first slot
                rank[l] += int((id_of_slot[max(s[l], d0 + 64):e[l]] < my[l]).sum())       # ... and behind its last one
        for l in range(GS.WAVE):
            if act[l]:
                assert order[s[l] + rank[l]] == -1, f"slot {s[l] + rank[l]} ranked twice (wave at {d0}, lane {l})"
                order[s[l] + rank[l]] = src[l]
    return order


def _sort_check(cells, ids, num_cells, want_counts, want_order, what):
    """Both emulations over `cells` in state order with particle ids `ids`; want_order in source indices."""
    for seed in ARRIVAL_SEEDS:
        key_cell, key_slot, count = emulate_bin(cells, num_cells, seed)
        assert np.array_equal(key_cell, cells), what
        assert np.array_equal(count, want_counts), f"{what}, arrival {seed}: counts"
        for c in np.nonzero(count)[0]:
            slots = np.sort(key_slot[cells == c])
            assert np.array_equal(slots, np.arange(count[c])), f"{what}, arrival {seed}: the slots of cell {c} are no permutation"
        cell_start = np.concatenate([[0], np.cumsum(count)])
        tmp = emulate_scatter(key_cell, key_slot, cell_start)
        order = emulate_rank(tmp, cell_start, ids, num_cells)
        assert np.array_equal(order, want_order), f"{what}, arrival {seed}: order"


def _oracle_grid(pkg, oracle, dims, cells, seed):
    rec, sp = GS.from_cells(pkg, dims, cells, seed)
    b = oracle.build_grid(rec, to_oracle_params(oracle, sp))
    assert tuple(b["grid"].dims) == tuple(dims)
    assert np.array_equal(b["particle_cell"], cells), "a particle is not in the cell the scene names"
    return b


SEQUENCES = GS.sequences()
LAYOUTS = GS.layouts()
NUM_CELLS = int(np.prod(GS.RUN_DIMS))


@pytest.mark.parametrize("name", sorted(SEQUENCES) + sorted(LAYOUTS))
def test_first_build_and_the_build_after_it(pkg, oracle, name):
    """The first build (state in upload order, id = index) and the build of the next substep (state in sorted order, the ids a
    permutation): counts, slots and order against the oracle's stable counting sort."""
    cells = SEQUENCES[name] if name in SEQUENCES else LAYOUTS[name][2]
    b = _oracle_grid(pkg, oracle, GS.RUN_DIMS, cells, 3)
    counts, order = np.diff(b["cell_start"]).astype(np.int64), b["order"].astype(np.int64)
    assert np.array_equal(order, np.lexsort((np.arange(len(cells)), cells)))            # the stable sort by (cell, id)
    _sort_check(cells, np.arange(len(cells)), NUM_CELLS, counts, order, name + " first build")
    # the next substep: slot s holds particle order[s]; sorted again, the state does not move
    _sort_check(cells[order], order, NUM_CELLS, counts, np.arange(len(cells)), name + " sorted state")


def test_rank_alone_on_a_reversed_arrival(pkg, oracle):
    """k_rank's input with every cell's members in DESCENDING id (the worst arrival): every rank is moved."""
    counts, first, cells = LAYOUTS["table300"]
    n = len(cells)
    want = np.lexsort((np.arange(n), cells))
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=NUM_CELLS))])
    rev = np.lexsort((-np.arange(n), cells))
    tmp = np.stack([rev, cells[rev]], axis=1)
    assert np.array_equal(emulate_rank(tmp, cell_start, np.arange(n), NUM_CELLS), want)


# ---- the scenes reach what they claim ------------------------------------------------------------------
def test_run_table_is_complete():
    seq = SEQUENCES["runs"]
    assert len(seq) < 25000 and len(seq) % GS.WAVE and len(seq) % GS.BLOCK
    got = {(a % GS.WAVE, length) for a, length, _ in GS.runs_of(seq)}
    missing = [(lane, length) for length in GS.RUN_LENGTHS for lane in GS.RUN_LANES if (lane, length) not in got]
    assert not missing, missing
    own = set(GS.spaced_cells(GS.RUN_DIMS).tolist())
    long_cells = [c for _, length, c in GS.runs_of(seq) if length > 1]
    assert len(long_cells) == len(set(long_cells)) and set(long_cells) <= own           # every long run has a cell of its own


@pytest.mark.parametrize("K", GS.ROUND_ROBIN_K)
def test_round_robin_feeds_every_cell_from_every_wave(K):
    seq = SEQUENCES[f"round_robin{K}"]
    assert all(length == 1 for _, length, _ in GS.runs_of(seq))                          # every lane is a head
    waves = [set(seq[w:w + GS.WAVE].tolist()) for w in range(0, len(seq), GS.WAVE)]
    want = set(seq.tolist())
    assert len(want) == K and len(waves) > 2 * GS.BLOCK // GS.WAVE
    assert all(len(w) == min(K, GS.WAVE) for w in waves[:-1])                            # a wave feeds as many cells as it has lanes
    blocks = [set(seq[b:b + GS.BLOCK].tolist()) for b in range(0, len(seq), GS.BLOCK)]
    assert all(b == want for b in blocks)                                                # every block feeds every cell, the last one too
    if K == 2:
        assert np.bincount(seq).max() == 1750 > GS.BLOCK


def test_revisit_and_descending_shapes():
    seq = SEQUENCES["revisit"]
    A = int(seq[0])
    starts = [a for a, _, c in GS.runs_of(seq) if c == A]
    assert sum(a < GS.WAVE for a in starts) >= 2                                         # two separate runs inside wave 0
    assert len({a // GS.BLOCK for a in starts}) >= 3                                     # and again in later blocks
    assert any(a // GS.WAVE != (a + length - 1) // GS.WAVE for a, length, c in GS.runs_of(seq) if c == A)    # a run across a wave seam
    d = [c for _, _, c in GS.runs_of(SEQUENCES["descending"])]
    assert len(d) > 300 and all(x > y for x, y in zip(d, d[1:]))


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_alignment_table_is_complete(name):
    counts, first, cells = LAYOUTS[name]
    n = len(cells)
    assert n == counts.sum() and n % GS.WAVE and n % GS.BLOCK
    start = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(np.bincount(cells - first, minlength=len(counts)), counts)
    got = {(int(m), int(s) % GS.WAVE) for m, s in zip(counts, start[:-1])}
    missing = [(m, o) for m in GS.LAYOUT_SIZES for o in GS.LAYOUT_OFFSETS if (m, o) not in got]
    assert not missing, missing
    spans = [(int(s), int(s + m)) for m, s in zip(counts, start[:-1]) if m]
    # the historic case: more than 64 members, beginning in front of the first slot of a wave the cell reaches into
    assert any(e - s > 64 and s % GS.WAVE and (s // GS.WAVE + 1) * GS.WAVE < e for s, e in spans)
    assert any((e - 1) // GS.WAVE - s // GS.WAVE >= 2 for s, e in spans)                 # a cell over three waves
    assert any(s // GS.BLOCK != (e - 1) // GS.BLOCK for s, e in spans)                   # a cell across a 256-slot boundary
    assert spans[-1][1] == n and spans[-1][1] - spans[-1][0] > 64                        # a crowded cell ends exactly at slot n
    assert (counts == 0).any()                                                           # empty cells between occupied ones
    assert (np.diff(cells) != 0).mean() > 0.9                                            # the arrival order is shuffled


def test_grid_facts(pkg):
    for dims in GS.SMALL_GRIDS + GS.LARGE_GRIDS:
        cells, residue, n_tiles = GS.GRID_FACTS[dims]
        assert int(np.prod(dims)) == cells and cells % GS.SCAN_ITEMS == residue and GS.tiles(cells) == n_tiles, dims
        sp = GS.params(pkg, dims)                                                        # asserts the dims
        assert pkg.compute_grid_extents(sp).numCells == cells
    assert GS.tiles(128 ** 3) == GS.SCAN_FUSED and GS.tiles(160 * 160 * 82) == GS.SCAN_FUSED + 1 == GS.tiles(119 * 125 * 141)
    assert -(-(GS.SCAN_FUSED + 1) // GS.BLOCK) == 5                                      # k_scan_blocksums: carry over five chunks of 256
    for axis in range(3):
        rec, sp, patches = GS.axis_patches(pkg, axis)
        assert pkg.compute_grid_extents(sp).dims[axis] == 1024


@pytest.mark.parametrize("dims", GS.SMALL_GRIDS + GS.LARGE_GRIDS)
def test_seam_scenes_occupy_the_seams(pkg, oracle, dims):
    C = int(np.prod(dims))
    cells = GS.seam_scene_cells(dims, 7)
    b = _oracle_grid(pkg, oracle, dims, cells, 7)
    cnt = np.diff(b["cell_start"])
    assert cnt[0] >= 2 and cnt[C - 1] >= 2
    if C <= 2 * GS.SCAN_TILE:
        s = np.arange(GS.SCAN_ITEMS, C, GS.SCAN_ITEMS)
        assert (cnt[s - 1] >= 2).all() and (cnt[s] >= 2).all()
    else:
        s = np.arange(GS.SCAN_TILE, C, GS.SCAN_TILE)                                     # every tile seam
        assert len(s) == GS.tiles(C) - 1 and (cnt[s - 1] >= 2).all() and (cnt[s] >= 2).all()
        for t in GS.NAMED_TILES + (GS.tiles(C) - 1,):                                    # the thread seams at both ends of the named tiles
            lo, hi = t * GS.SCAN_TILE, min((t + 1) * GS.SCAN_TILE, C)
            last = lo + (hi - 1 - lo) // GS.SCAN_ITEMS * GS.SCAN_ITEMS
            assert (cnt[[lo + 7, lo + 8, last - 1, last]] >= 2).all() and cnt[lo:hi].sum() >= 8, (dims, t)
