"""Scenes for the tests of the counting sort (k_bin, k_scan_*, k_scatter, k_rank of csrc/sph_kernels.h): grids of chosen dimensions,
particles placed in chosen cells in a chosen upload order, and the cell sequences that pin which lanes of a wave are run heads in k_bin
and where a cell's slot range lies against the 64- and 256-slot boundaries in k_rank.  numpy only; `pkg` lends the record type, the
parameter struct and the host-side grid extents.

Particle i (id i in upload order) sits at a seeded point 5-95 % inside cell cells[i], so the caller controls k_bin's runs at the first
build exactly: lane (i mod 64) of wave (i div 64) sees cell cells[i]."""
import numpy as np

F = np.float32
H = 0.5
WAVE, BLOCK = 64, 256                    # wave size and kBlock of sph_kernels.h
SCAN_ITEMS, SCAN_TILE, SCAN_FUSED = 8, 2048, 1024     # kScanItems, kScanTile, kScanFusedBlocks

RUN_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
RUN_LANES = (0, 1, 31, 32, 62, 63)
ROUND_ROBIN_K = (2, 7, 64, 65)
LAYOUT_SIZES = (1, 2, 63, 64, 65, 128, 200, 300)
LAYOUT_OFFSETS = (0, 1, 31, 62, 63)
RUN_DIMS = (16, 16, 16)                  # 4096 cells, two scan tiles


def params(pkg, dims, cap=160):
    """Box container, no rotation, h = 0.5, boxHalf[a] = h ((d_a - 2) / 2 - 0.25): the grid has exactly `dims` cells
    (ext = half + h, dims = ceil(2 ext / h) = ceil(d - 0.5)).  The fluid has the rest spacing 0.8 h."""
    half = tuple(float(H * ((d - 2) / 2.0 - 0.25)) for d in dims)
    s = 0.8 * H
    sp = pkg.default_params(param_h=H, param_mass=float(F(1000.0 * s ** 3)), param_restDensity=1000.0, param_boxCenter=(0.0, 0.0, 0.0),
                            param_boxHalf=half, param_boxEulerDeg=(0.0, 0.0, 0.0), param_shapeType=0, grid_cap=max(cap, max(dims)))
    g = pkg.compute_grid_extents(sp)
    assert tuple(g.dims) == tuple(dims), (tuple(g.dims), dims)
    return sp


def records(pkg, pos):
    """Active fluid records at rest, at rest density."""
    rec = np.zeros(len(pos), pkg.PARTICLE_DTYPE)
    rec["pos"][:, :3] = pos
    rec["pos"][:, 3] = 1.0
    rec["density"] = 1000.0
    rec["isActive"] = 1
    return rec


def cell_points(pkg, sp, cells, seed):
    """One seeded point 5-95 % inside each of the flattened cells `cells` (float32, like the records)."""
    g = pkg.compute_grid_extents(sp)
    gx, gy, gz = (int(d) for d in g.dims)
    cells = np.asarray(cells, np.int64)
    assert len(cells) and cells.min() >= 0 and cells.max() < gx * gy * gz
    coord = np.stack([cells % gx, (cells // gx) % gy, cells // (gx * gy)], axis=1).astype(np.float64)
    u = 0.05 + 0.9 * np.random.default_rng(seed).random((len(cells), 3))
    return (np.array(list(g.gridMin), np.float64) + (coord + u) * float(g.cellSize)).astype(F)


def from_cells(pkg, dims, cells, seed, cap=160):
    """(records, params): particle i in cell cells[i] of a grid of `dims` cells."""
    sp = params(pkg, dims, cap)
    return records(pkg, cell_points(pkg, sp, cells, seed)), sp


# ---- cell sequences: which lanes are run heads in k_bin -----------------------------------------------
def spaced_cells(dims):
    """Cells whose coordinates are all 1 mod 3: no two of them are neighbours, so a neighbour row at 2 h around a member of one
    holds no member of another."""
    gx, gy, gz = dims
    return np.array([(z * gy + y) * gx + x for z in range(1, gz - 1, 3) for y in range(1, gy - 1, 3) for x in range(1, gx - 1, 3)], np.int64)


def _pads(dims, taken):
    """The cells that are no run cell, in a seeded order: consecutive pads differ, so every pad is a run of one."""
    free = np.setdiff1d(np.arange(int(np.prod(dims)), dtype=np.int64), taken)
    return free[np.random.default_rng(5).permutation(len(free))]


def runs_of(cells):
    """[(index of the first particle, length, cell)] of the maximal runs of equal consecutive cells."""
    cells = np.asarray(cells, np.int64)
    first = np.concatenate([[0], np.nonzero(np.diff(cells))[0] + 1])
    length = np.diff(np.concatenate([first, [len(cells)]]))
    return [(int(a), int(l), int(cells[a])) for a, l in zip(first, length)]


def runs(dims=RUN_DIMS):
    """Every run length of RUN_LENGTHS starting at every lane of RUN_LANES, each in a cell of its own, padded with runs of one."""
    own = spaced_cells(dims)
    assert len(own) >= len(RUN_LENGTHS) * len(RUN_LANES)
    pad = _pads(dims, own)
    seq, p, k = [], 0, 0
    for length in RUN_LENGTHS:
        for lane in RUN_LANES:
            while len(seq) % WAVE != lane:
                seq.append(pad[p % len(pad)])
                p += 1
            seq += [own[k]] * length
            k += 1
    while len(seq) % BLOCK < 70 or len(seq) % WAVE == 0:         # a partial last block of more than one wave, a partial last wave
        seq.append(pad[p % len(pad)])
        p += 1
    return np.array(seq, np.int64)


def round_robin(K, n=3500, dims=RUN_DIMS):
    """cells[i] = c[i mod K]: every lane is a head, every cell is fed by every wave of every block."""
    return spaced_cells(dims)[:K][np.arange(n) % K]


def revisit(dims=RUN_DIMS):
    """Cell A as two separate runs inside wave 0 (and B between them), A again across the seam of waves 1 and 2, A and B again in
    the second and third block."""
    own = spaced_cells(dims)
    A, B = own[3], own[4]
    pad = _pads(dims, own)
    seq = [A] * 10 + [B] * 5 + [A] * 10 + list(pad[:5]) + [B] * 3 + [A] * 1 + list(pad[5:35])        # wave 0
    seq += list(pad[35:95]) + [A] * 8                                                                # A: lanes 60-63 of wave 1, 0-3 of wave 2
    seq += list(pad[95:95 + 300 - len(seq)]) + [A] * 20 + [B] * 70 + [A] * 2                          # second block
    seq += list(pad[400:400 + 520 - len(seq)]) + [B] * 1 + [A] * 65 + list(pad[600:637])              # third block, partial last wave
    return np.array(seq, np.int64)


def descending(dims=RUN_DIMS, n=3000, seed=9):
    """Runs of 1-9 particles in falling cell order."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 10, n)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n))]
    cells = np.sort(rng.choice(int(np.prod(dims)), len(lengths), replace=False))[::-1]
    return np.repeat(cells, lengths).astype(np.int64)


def sequences():
    """{name: cells} of every first-build sequence."""
    out = {"runs": runs(), "revisit": revisit(), "descending": descending()}
    out.update({f"round_robin{K}": round_robin(K) for K in ROUND_ROBIN_K})
    return out


# ---- layouts: where a cell's slot range lies in k_rank ------------------------------------------------
def layout_counts(order_seed, last):
    """Member counts of consecutive cells in which a cell of every size of LAYOUT_SIZES begins at every slot offset of LAYOUT_OFFSETS
    mod 64, in a seeded order of the (size, offset) pairs; small cells (0-5 members) in between move the next one to its offset.  The
    last cell has `last` members and ends at slot n."""
    rng = np.random.default_rng(order_seed)
    pairs = [(m, o) for m in LAYOUT_SIZES for o in LAYOUT_OFFSETS]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    counts, cur = [], 0
    for m, o in pairs + [(last, 62)]:
        gap = (o - cur) % WAVE
        while gap:
            c = int(min(gap, rng.integers(0, 6)))
            counts.append(c)
            gap -= c
            cur += c
        counts.append(m)
        cur += m
    return np.array(counts, np.int64)


def layout(counts, seed, first_cell=0):
    """cells[i] of a seeded upload order in which cell first_cell + k has counts[k] members: the sorted slot ranges are
    cumsum(counts), the arrival order is arbitrary."""
    sorted_cells = np.repeat(first_cell + np.arange(len(counts), dtype=np.int64), counts)
    return sorted_cells[np.random.default_rng(seed).permutation(len(sorted_cells))]


def layouts():
    """{name: (counts, first cell, cells)}: the alignment table twice, in two orders, ending in a cell of 300 and in one of 65."""
    out = {}
    for name, order_seed, last, first in (("table300", 21, 300, 0), ("table65", 22, 65, 517)):
        counts = layout_counts(order_seed, last)
        out[name] = (counts, first, layout(counts, order_seed + 100, first))
    return out


# ---- scan seams ----------------------------------------------------------------------------------------
SMALL_GRIDS = ((3, 5, 136), (4, 7, 73), (3, 11, 62), (4, 4, 128), (5, 5, 82), (3, 5, 137), (3, 29, 47), (3, 13, 105), (4, 8, 128), (3, 3, 3))
LARGE_GRIDS = ((128, 128, 128), (160, 160, 82), (119, 125, 141))
# (cells, cells mod 8, scan tiles) as the issue of this suite states them
GRID_FACTS = {(3, 5, 136): (2040, 0, 1), (4, 7, 73): (2044, 4, 1), (3, 11, 62): (2046, 6, 1), (4, 4, 128): (2048, 0, 1),
              (5, 5, 82): (2050, 2, 2), (3, 5, 137): (2055, 7, 2), (3, 29, 47): (4089, 1, 2), (3, 13, 105): (4095, 7, 2),
              (4, 8, 128): (4096, 0, 2), (3, 3, 3): (27, 3, 1), (128, 128, 128): (2097152, 0, 1024), (160, 160, 82): (2099200, 0, 1025),
              (119, 125, 141): (2097375, 7, 1025)}
NAMED_TILES = (0, 255, 256, 257, 511, 512, 1023)         # and the last one


def tiles(num_cells):
    return -(-num_cells // SCAN_TILE)


def seam_cells(num_cells):
    """The cells that get explicit members: cell 0, the last cell and both sides of every seam.  Up to 4096 cells that is every 8-cell
    thread seam (so every tile seam too).  A grid of two million cells has 262 144 thread seams, more than the scene has particles:
    there the cells are both sides of every tile seam, and inside the named tiles (0, 255, 256, 257, 511, 512, 1023, the last) both
    sides of the first and of the last thread seam."""
    C = num_cells
    if C <= 2 * SCAN_TILE:
        s = np.arange(SCAN_ITEMS, C, SCAN_ITEMS)
        cells = np.concatenate([[0, C - 1], s - 1, s])
    else:
        s = np.arange(SCAN_TILE, C, SCAN_TILE)
        cells = [0, C - 1]
        for t in NAMED_TILES + (tiles(C) - 1,):
            lo, hi = t * SCAN_TILE, min((t + 1) * SCAN_TILE, C)
            last = lo + (hi - 1 - lo) // SCAN_ITEMS * SCAN_ITEMS                  # first cell of the tile's last thread
            cells += [lo + SCAN_ITEMS - 1, lo + SCAN_ITEMS, last - 1, last]
        cells = np.concatenate([cells, s - 1, s])
    return np.unique(cells[(cells >= 0) & (cells < C)]).astype(np.int64)


def seam_scene_cells(dims, seed):
    """About 4000 (small grids) or 20 000 (large grids) uniformly chosen cells, then two members of every seam cell, shuffled."""
    C = int(np.prod(dims))
    rng = np.random.default_rng(seed)
    cells = np.concatenate([rng.integers(0, C, 4000 if C <= 2 * SCAN_TILE else 20000), np.repeat(seam_cells(C), 2)])
    return cells[rng.permutation(len(cells))]


# ---- axis limits ---------------------------------------------------------------------------------------
def axis_patches(pkg, axis, length=1024):
    """(records, params, [index arrays]): a grid of `length` cells along `axis` and 3 on the others, with three lattice patches of
    spacing 0.8 h (3 x 3 particles across) over cells 0..2, 510..513 and 1021..1023 of the long axis."""
    dims = [3, 3, 3]
    dims[axis] = length
    sp = params(pkg, tuple(dims), cap=length)
    g = pkg.compute_grid_extents(sp)
    lo, cs, s = float(g.gridMin[axis]), float(g.cellSize), 0.8 * H
    pos, patches = [], []
    for first, last in ((0, 2), (length // 2 - 2, length // 2 + 1), (length - 3, length - 1)):
        a = lo + first * cs + 0.05 + s * np.arange(int(((last + 1 - first) * cs - 0.1) / s) + 1)
        assert a[-1] < lo + (last + 1) * cs
        across = s * np.array([-1.0, 0.0, 1.0])
        p = np.zeros((len(a) * 9, 3))
        p[:, axis] = np.repeat(a, 9)
        p[:, (axis + 1) % 3] = np.tile(np.repeat(across, 3), len(a))
        p[:, (axis + 2) % 3] = np.tile(across, 3 * len(a))
        patches.append(np.arange(len(p)) + sum(len(q) for q in pos))
        pos.append(p)
    return records(pkg, np.concatenate(pos).astype(F)), sp, patches
