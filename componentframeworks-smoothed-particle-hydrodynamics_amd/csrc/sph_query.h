// sph_query.h -- what the spatial queries share (neighbour lists, components, kNN, shell, aniso, rays; the *_host twins): the stencil
// and its row walk, the candidate walk of the families that sum over positions alone (shell, aniso), the target of a lane, the CPU grid
// of the twins, and the kernels every family launches.  Shared layer (with sph_sample.h): it stands on the base and substep headers
// only, and every feature header may include it.
//
// A target at x in cell (cx, cy, cz) (cell_of, clamped) sees the members of the cells [c - s, c + s] per axis that lie in the grid,
// s = 1, 2, 3 the smallest half-width with R <= (float)s * cellSize: (2s + 1)^2 rows in (dz, dy) order, each row one contiguous run of
// sorted slots, i.e. ascending sorted slot = ascending (cell index, particle id).
//
//   neighbor_stencil / neighbor_rows / neighbor_accept / neighbor_offset: __host__ __device__ (the twins walk HostGrid with them);
//   slot_ghost / query_target: device
//   neighbor_gather<SKIP> / HostGrid::gather: the candidate walk of the shell's pass 1 and the aniso gather, device and twin.  The other
//                          families keep their loops: they read other data before the distance test, keep j, or stage rows in LDS.
// The kernels keep the names of their first users (tools and committed profiles match kernels by name); all of them are shared:
//   k_neighbors_ids        ids[slot] = particle id of the sorted slot (neighbour lists, kNN, shell)
//   k_neighbors_scan_*     64-bit exclusive scan of cnt into offsets[0 .. rows], and the largest count; tiles, no atomics (neighbour
//                          lists, components, shell)
//   k_shell_compact        out[offsets[i]] = i where flag[i]: the second half of a compaction behind that scan
#pragma once
#include <vector>

#include "../../include/sph_abi.h"
#include "sph_kernels.h"

namespace sph {

constexpr int kNbMaxStencil = 3;
// Smallest half-width s in 1 .. 3 with R <= (float)s * cellSize; 0: R is not a radius (not finite, <= 0, above three cells).
__host__ __device__ inline int neighbor_stencil(float R, float cellSize) {
    if (!(R > 0.0f) || !(R <= 3.0f * cellSize)) return 0;
    for (int s = 1; s <= kNbMaxStencil; ++s)
        if (R <= (float)s * cellSize) return s;
    return 0;
}

// Is candidate j inside the radius of the target?  dot3 of sph_device.h for both sides; NaN on either side rejects.
__host__ __device__ inline bool neighbor_accept(float xi, float yi, float zi, float xj, float yj, float zj, float R2) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return dot3(dx, dy, dz, dx, dy, dz) < R2;
}
// The same test for a family that sums over d = x_j - x: r2 = dot3(d, d) has the bits of neighbor_accept's r2 (its d is the exact
// negative, the squares are the same floats).
__host__ __device__ inline bool neighbor_offset(float xi, float yi, float zi, float xj, float yj, float zj, float R2, float& dx, float& dy, float& dz, float& r2) {
    dx = xj - xi; dy = yj - yi; dz = zj - zi;
    r2 = dot3(dx, dy, dz, dx, dy, dz);
    return r2 < R2;
}

struct NbK {
    float R2;
    int s, flags;
    uint32_t idBase, n;
};

// sample_rows at half-width s: f(first slot, end slot) per row that lies inside the grid, in ascending slot order.  __host__ too: the
// *_host references walk their grid (HostGrid) with this very function.
template <class F>
__host__ __device__ __forceinline__ void neighbor_rows(const SimK& k, const uint32_t* __restrict__ cellStart, int s, uint32_t n, int cx, int cy, int cz, F&& f) {
    const int xlo = max(cx - s, 0), xhi = min(cx + s, k.gx - 1), w = 2 * s + 1;
    for (int r = 0; r < w * w; ++r) {
        const int nz = cz + r / w - s, ny = cy + r % w - s;
        if (nz < 0 || nz >= k.gz || ny < 0 || ny >= k.gy) continue;
        const int rowBase = (nz * k.gy + ny) * k.gx;
        f(cellStart[rowBase + xlo], min(cellStart[rowBase + xhi + 1], n));
    }
}

// Is the record of sorted slot j a ghost (isGhost != 0)?  One word of its own data.
__device__ __forceinline__ bool slot_ghost(const float4* __restrict__ own, uint32_t j) {
    return (fbits(reinterpret_cast<const float*>(own)[(size_t)j * 4u + 2u]) & F_GHOSTNZ) != 0u;
}

// The candidate walk of a target at P: f(dx, dy, dz, r2) per accepted candidate j of the rows of cell_of(P), j ascending, without
// j == self where SKIP; under fluidOnly without ghosts.  The position is loaded first, the own data second and for accepted candidates only.
template <bool SKIP, class F>
__device__ __forceinline__ void neighbor_gather(const SimK& k, const NbK& nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                const float4* __restrict__ own, bool fluidOnly, const float4& P, uint32_t self, F&& f) {
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            if (SKIP && j == self) continue;
            const float4 J = pv[2u * j];
            float dx, dy, dz, r2;
            if (!neighbor_offset(P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2)) continue;
            if (fluidOnly && slot_ghost(own, j)) continue;
            f(dx, dy, dz, r2);
        }
    });
}

// The grid of host records as the counting sort leaves it: cells ascending, members ascending by index.  start[c] is the first sorted
// slot of cell c, order[slot] the record in that slot, slotOf[i] the slot of record i.  Every *_host reference builds this one and
// walks it with the device's own neighbor_rows.
struct HostGrid {
    const SimK& k;
    std::vector<uint32_t> start, order, slotOf;
    HostGrid(const SimK& k_, const SphParticle* particles, size_t n) : k(k_), start((size_t)k_.numCells + 1, 0u), order(n), slotOf(n) {
        std::vector<uint32_t> cellOf(n);
        for (size_t i = 0; i < n; ++i) {
            const int3 c = cell_of(k, particles[i].pos[0], particles[i].pos[1], particles[i].pos[2]);
            cellOf[i] = (uint32_t)((c.z * k.gy + c.y) * k.gx + c.x);
            start[cellOf[i] + 1] += 1u;
        }
        for (size_t c = 0; c < (size_t)k.numCells; ++c) start[c + 1] += start[c];
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < n; ++i) { slotOf[i] = fill[cellOf[i]]++; order[slotOf[i]] = (uint32_t)i; }
    }
    // f(first slot, end slot) per in-grid row of the (2s + 1)^2 around a cell, or around the clamped cell of a point, in ascending slot order.
    template <class F>
    void rows(int s, int cx, int cy, int cz, F&& f) const { neighbor_rows(k, start.data(), s, (uint32_t)order.size(), cx, cy, cz, f); }
    template <class F>
    void rows(int s, const float* x, F&& f) const { const int3 c = cell_of(k, x[0], x[1], x[2]); rows(s, c.x, c.y, c.z, f); }
    // neighbor_gather's twin for a target at x: the same visits in the same order over order[]; skipSlot is kNoSlot where nothing is skipped.
    static constexpr uint32_t kNoSlot = 0xffffffffu;
    template <class F>
    void gather(int s, const float* x, float R2, const SphParticle* particles, bool fluidOnly, uint32_t skipSlot, F&& f) const {
        rows(s, x, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                if (j == skipSlot) continue;
                const SphParticle& c = particles[order[j]];
                float dx, dy, dz, r2;
                if (!neighbor_offset(x[0], x[1], x[2], c.pos[0], c.pos[1], c.pos[2], R2, dx, dy, dz, r2)) continue;
                if (fluidOnly && c.isGhost != 0) continue;
                f(dx, dy, dz, r2);
            }
        });
    }
};

// Target of a lane: particle rows, slot i -> (position, row = id); query rows, point i -> (position, row = i).  false: the lane has no
// row.  walk: a query point walks when it is finite; a particle always does.  A family's FLUID_ONLY rule for a ghost target stays with
// the family: as an argument here it cost k_knn and k_shell_gather 0.3 to 2.6 % (profiles/r20_header_refactor_ab.json).
template <bool PARTICLES>
__device__ __forceinline__ bool query_target(const float4* __restrict__ pv, const int32_t* __restrict__ ids, const float4* __restrict__ points, size_t rows,
                                             size_t i, float4& P, size_t& row, bool& walk) {
    if (i >= rows) return false;
    if (PARTICLES) {
        P = pv[2u * (uint32_t)i];
        row = (size_t)(uint32_t)ids[i];
        walk = true;
        return row < rows;
    }
    P = points[i];
    row = i;
    walk = sample_finite(P.x, P.y, P.z);
    return true;
}

__global__ __launch_bounds__(kBlock) void k_neighbors_ids(const float4* __restrict__ own, int32_t* __restrict__ ids, uint32_t idBase, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const uint32_t id = fbits(own[q].w) - idBase;
    ids[q] = id < n ? (int32_t)id : 0;
}

// ---- 64-bit exclusive scan of cnt[0 .. rows) into offsets[0 .. rows], and max(cnt) ----------------------------------------------
// Tiles of kScanTile counts as the grid's scan: per-tile sums and maxima, one block scans the tile sums (chunks of 256 with a carry),
// then every tile scans its own counts behind its offset.  totals[0] = the sum, totals[1] = the largest count.
__global__ __launch_bounds__(kBlock) void k_neighbors_scan_reduce(const uint32_t* __restrict__ cnt, size_t rows, unsigned long long* __restrict__ tileSums,
                                                                  uint32_t* __restrict__ tileMax) {
    __shared__ unsigned long long sm[4];
    __shared__ uint32_t smx[4];
    const size_t c0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    unsigned long long s = 0ull;
    uint32_t mx = 0u;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        const uint32_t v = (c0 + j < rows) ? cnt[c0 + j] : 0u;
        s += v;
        mx = max(mx, v);
    }
    unsigned long long total;
    (void)block_excl_scan64(s, sm, total);
    mx = block_max(mx, smx);
    if (threadIdx.x == 0) { tileSums[blockIdx.x] = total; tileMax[blockIdx.x] = mx; }
}

// single block
__global__ __launch_bounds__(kBlock) void k_neighbors_scan_tiles(unsigned long long* __restrict__ tileSums, const uint32_t* __restrict__ tileMax, int tiles,
                                                                 unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long sm[4];
    __shared__ uint32_t smx[4];
    unsigned long long carry = 0ull;
    uint32_t mx = 0u;
    for (int base = 0; base < tiles; base += kBlock) {
        const int i = base + threadIdx.x;
        const unsigned long long v = (i < tiles) ? tileSums[i] : 0ull;
        mx = max(mx, (i < tiles) ? tileMax[i] : 0u);
        unsigned long long total;
        const unsigned long long ex = block_excl_scan64(v, sm, total);
        if (i < tiles) tileSums[i] = carry + ex;
        carry += total;
    }
    mx = block_max(mx, smx);
    if (threadIdx.x == 0) { totals[0] = carry; totals[1] = mx; }
}

__global__ __launch_bounds__(kBlock) void k_neighbors_scan_apply(const uint32_t* __restrict__ cnt, size_t rows, const unsigned long long* __restrict__ tileSums,
                                                                 const unsigned long long* __restrict__ totals, long long* __restrict__ offsets) {
    __shared__ unsigned long long sm[4];
    const size_t c0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    unsigned long long v[kScanItems], s = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) { const uint32_t t = (c0 + j < rows) ? cnt[c0 + j] : 0u; v[j] = s; s += t; }     // exclusive prefix inside the thread
    unsigned long long total;
    const unsigned long long off = tileSums[blockIdx.x] + block_excl_scan64(s, sm, total);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) if (c0 + j < rows) offsets[c0 + j] = (long long)(off + v[j]);
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[rows] = (long long)totals[0];
}

// The second half of a compaction: out[offsets[i]] = i where flag[i] (offsets: the exclusive scan of flag).
__global__ __launch_bounds__(kBlock) void k_shell_compact(const uint32_t* __restrict__ flag, const long long* __restrict__ offsets, size_t rows,
                                                          int32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows || !flag[i]) return;
    const long long at = offsets[i];
    if (at >= 0 && (size_t)at < rows) out[at] = (int32_t)i;
}

}  // namespace sph
