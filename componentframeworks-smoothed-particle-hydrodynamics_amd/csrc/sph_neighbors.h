// sph_neighbors.h -- fixed-radius neighbour lists in CSR form, of the particles or of query points (no reference counterpart;
// DESIGN.md section 3k).
//
// A target at x in cell (cx, cy, cz) (BuildGrid's formula, clamped) sees the members of the cells [c - s, c + s] per axis that lie in
// the grid, s = 1, 2, 3 the smallest half-width with R <= (float)s * cellSize: (2s + 1)^2 rows in (dz, dy) order, each row one
// contiguous run of sorted slots, i.e. ascending sorted slot = ascending (cell index, particle id).  Candidate j is accepted when
// r2 < R2, r2 the fma-based dot3 of x - x_j (sweep 1's test at R = h).  Everything is integer from there on.
//
//   neighbor_accept / neighbor_keep   the per-candidate test, __host__ __device__: sph_neighbors_host runs the same functions
//   k_neighbors_ids        ids[slot] = particle id of the sorted slot (4 bytes per slot instead of a 16-byte own record per entry)
//   k_neighbors_count<P>   one target per lane (P: sorted-slot order, rows numbered by id; else the caller's points), cnt[row]
//   k_neighbors_scan_*     64-bit exclusive scan of cnt into offsets[0 .. rows], and the largest count; tiles, no atomics
//   k_neighbors_fill<P>    the same walk; lane-owned stores indices[offsets[row] + running]
//   k_neighbors_fill_wave<P>   the A/B variant of the fill (SPH_OPT_NEIGHBORS_FILL 1): a wave writes one row at a time, same bits
// Ids are a permutation of [0, n), cellStart ends at n and the fill finds what the count found, so the range guards in these kernels
// (id < n, row < rows, min(cellStart, n), w < end) never fire; they stay so that no load or store can leave its array.
// Candidate rows are read straight from global memory (the LDS-staged scalar sweep lost to the plain walk).
#pragma once
#include <math.h>

#include "sph_surface.h"   // sample_finite of sph_sample.h, wave_incl_scan64

namespace sph {

constexpr int kNbSelf = 1, kNbHalf = 2, kNbCountOnly = 4;      // SPH_NEIGHBORS_* of sph_abi.h
constexpr int kNbMaxStencil = 3;

// Is candidate j inside the radius of the target?  dot3 of sph_device.h for both sides; NaN on either side rejects.
__host__ __device__ inline bool neighbor_accept(float xi, float yi, float zi, float xj, float yj, float zj, float R2) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const float r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    return r2 < R2;
}
// Does an entry of a PARTICLE list stay?  own: the candidate is the target's own slot (kept by identity under SELF, never otherwise).
__host__ __device__ inline bool neighbor_keep(int flags, bool own, bool accepted, uint32_t idTarget, uint32_t idCandidate) {
    if (own) return (flags & kNbSelf) != 0;
    return accepted && (!(flags & kNbHalf) || idCandidate > idTarget);
}
// Smallest half-width s in 1 .. 3 with R <= (float)s * cellSize; 0: R is not a radius (not finite, <= 0, above three cells).
__host__ __device__ inline int neighbor_stencil(float R, float cellSize) {
    if (!(R > 0.0f) || !(R <= 3.0f * cellSize)) return 0;
    for (int s = 1; s <= kNbMaxStencil; ++s)
        if (R <= (float)s * cellSize) return s;
    return 0;
}

struct NbK {
    float R2;
    int s, flags;
    uint32_t idBase, n;
};

// sample_rows at half-width s: f(first slot, end slot) per row that lies inside the grid, in ascending slot order.  __host__ too: the
// *_host references walk their grid (HostGrid of sph_scalar.h) with this very function.
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

__global__ __launch_bounds__(kBlock) void k_neighbors_ids(const float4* __restrict__ own, int32_t* __restrict__ ids, uint32_t idBase, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const uint32_t id = fbits(own[q].w) - idBase;
    ids[q] = id < n ? (int32_t)id : 0;
}

// The walk of one target: emit(id of the kept candidate) per entry, in order.  q: the target's own slot (particle lists).
template <bool PARTICLES, class E>
__device__ __forceinline__ void neighbor_walk(const SimK& k, const NbK& nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                              const int32_t* __restrict__ ids, float px, float py, float pz, uint32_t q, uint32_t idTarget, E&& emit) {
    const int cx = cell_axis(px, k.gminx, k.cellSize, k.gx), cy = cell_axis(py, k.gminy, k.cellSize, k.gy), cz = cell_axis(pz, k.gminz, k.cellSize, k.gz);
    const bool half = (nb.flags & kNbHalf) != 0;
    neighbor_rows(k, cellStart, nb.s, nb.n, cx, cy, cz, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            const float4 J = pv[2u * j];
            const bool acc = neighbor_accept(px, py, pz, J.x, J.y, J.z, nb.R2);
            if (PARTICLES) {
                const bool own = j == q;
                if (!own && !acc) continue;
                const uint32_t idj = (half && !own) ? (uint32_t)ids[j] : 0u;
                if (neighbor_keep(nb.flags, own, acc, idTarget, idj)) emit(j);
            } else if (acc) {
                emit(j);
            }
        }
    });
}

// Target of a lane: particle lists, slot q -> (position, row = id); query lists, point i -> (position, row = i).  false: no walk.
template <bool PARTICLES>
__device__ __forceinline__ bool neighbor_target(const NbK& nb, const float4* __restrict__ pv, const int32_t* __restrict__ ids,
                                                const float4* __restrict__ points, size_t rows, size_t i, float4& P, size_t& row, bool& walk) {
    if (i >= rows) return false;
    if (PARTICLES) {
        P = pv[2u * (uint32_t)i];
        row = (size_t)(uint32_t)ids[i];
        walk = true;                                                          // (a non-finite target accepts nobody but may keep itself)
        return row < rows;
    }
    P = points[i];
    row = i;
    walk = sample_finite(P.x, P.y, P.z);
    return true;
}

template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_neighbors_count(SimK k, NbK nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                            const int32_t* __restrict__ ids, const float4* __restrict__ points, size_t rows,
                                                            uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    size_t row;
    bool walk;
    if (!neighbor_target<PARTICLES>(nb, pv, ids, points, rows, i, P, row, walk)) return;
    uint32_t c = 0u;
    if (walk) neighbor_walk<PARTICLES>(k, nb, pv, cellStart, ids, P.x, P.y, P.z, (uint32_t)i, (uint32_t)row, [&](uint32_t) { c += 1u; });
    cnt[row] = c;
}

template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_neighbors_fill(SimK k, NbK nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                           const int32_t* __restrict__ ids, const float4* __restrict__ points, size_t rows,
                                                           const long long* __restrict__ offsets, int32_t* __restrict__ indices) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    size_t row;
    bool walk;
    if (!neighbor_target<PARTICLES>(nb, pv, ids, points, rows, i, P, row, walk) || !walk) return;
    long long w = offsets[row];
    const long long end = offsets[row + 1];
    neighbor_walk<PARTICLES>(k, nb, pv, cellStart, ids, P.x, P.y, P.z, (uint32_t)i, (uint32_t)row, [&](uint32_t j) {
        if (w < end) indices[w] = ids[j];
        w += 1;
    });
}

// The wave-cooperative row write (SPH_OPT_NEIGHBORS_FILL 1): a wave owns 64 consecutive targets and takes them one after the other;
// its lanes test 64 consecutive candidate slots of a row run at a time, and the kept ids leave as one run of consecutive words
// (ballot, prefix count).  Same tests in the same slot order, therefore the same bits as k_neighbors_fill.
template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_neighbors_fill_wave(SimK k, NbK nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                                const int32_t* __restrict__ ids, const float4* __restrict__ points, size_t rows,
                                                                const long long* __restrict__ offsets, int32_t* __restrict__ indices) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const size_t i0 = i - (size_t)lane;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    size_t row = 0;
    bool walk = false;
    const bool mine = neighbor_target<PARTICLES>(nb, pv, ids, points, rows, i, P, row, walk) && walk;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool half = (nb.flags & kNbHalf) != 0;
    for (int t = 0; t < 64; ++t) {                                            // every lane of the wave stays to the end: the targets cross the lanes
        if (!__shfl((int)mine, t, 64)) continue;                             // (wave-uniform)
        const float px = __shfl(P.x, t, 64), py = __shfl(P.y, t, 64), pz = __shfl(P.z, t, 64);
        const uint32_t trow = (uint32_t)__shfl((int)(uint32_t)row, t, 64);   // (rows < 2^31)
        const uint32_t q = (uint32_t)(i0 + (size_t)t);
        long long w = offsets[trow];
        const long long end = offsets[(size_t)trow + 1];
        const int cx = cell_axis(px, k.gminx, k.cellSize, k.gx), cy = cell_axis(py, k.gminy, k.cellSize, k.gy), cz = cell_axis(pz, k.gminz, k.cellSize, k.gz);
        neighbor_rows(k, cellStart, nb.s, nb.n, cx, cy, cz, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j0 = qs; j0 < qe; j0 += 64u) {
                const uint32_t j = j0 + (uint32_t)lane;
                bool keep = false;
                int32_t idj = 0;
                if (j < qe) {
                    const float4 J = pv[2u * j];
                    const bool acc = neighbor_accept(px, py, pz, J.x, J.y, J.z, nb.R2);
                    const bool own = PARTICLES && j == q;
                    if (own || acc) {
                        idj = ids[j];
                        keep = PARTICLES ? neighbor_keep(nb.flags, own, acc, trow, (half && !own) ? (uint32_t)idj : 0u) : acc;
                    }
                }
                const unsigned long long kept = __ballot(keep);
                const long long at = w + (long long)__popcll(kept & below);
                if (keep && at < end) indices[at] = idj;
                w += (long long)__popcll(kept);
            }
        });
    }
}

// ---- 64-bit exclusive scan of cnt[0 .. rows) into offsets[0 .. rows], and max(cnt) ----------------------------------------------
// Tiles of kScanTile counts as the grid's scan: per-tile sums and maxima, one block scans the tile sums (chunks of 256 with a carry),
// then every tile scans its own counts behind its offset.  totals[0] = the sum, totals[1] = the largest count.
__device__ __forceinline__ unsigned long long block_excl_scan64(unsigned long long v, unsigned long long* sm, unsigned long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long inc = wave_incl_scan64(v);
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    const unsigned long long w0 = sm[0], w1 = sm[1], w2 = sm[2], w3 = sm[3];
    const unsigned long long base = (w > 0 ? w0 : 0ull) + (w > 1 ? w1 : 0ull) + (w > 2 ? w2 : 0ull);
    total = w0 + w1 + w2 + w3;
    __syncthreads();
    return base + inc - v;
}
__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* sm) {
    for (int sh = 32; sh >= 1; sh >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, sh, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    __syncthreads();
    return m;
}

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

}  // namespace sph
