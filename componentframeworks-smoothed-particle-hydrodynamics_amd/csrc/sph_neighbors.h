// sph_neighbors.h -- fixed-radius neighbour lists in CSR form, of the particles or of query points (no reference counterpart;
// DESIGN.md section 3k).
//
// Stencil, candidate rows and the target of a lane are sph_query.h's (neighbor_stencil, neighbor_rows, query_target).  Candidate j is
// accepted when r2 < R2, r2 the fma-based dot3 of x - x_j (sweep 1's test at R = h).  Everything is integer from there on.
//
//   neighbor_accept (sph_query.h) / neighbor_keep   the per-candidate test, __host__ __device__: sph_neighbors_host runs the same functions
//   k_neighbors_ids        (sph_query.h) ids[slot] = particle id of the sorted slot (4 bytes per slot instead of a 16-byte own record per entry)
//   k_neighbors_count<P>   one target per lane (P: sorted-slot order, rows numbered by id; else the caller's points), cnt[row]
//   k_neighbors_scan_*     (sph_query.h) 64-bit exclusive scan of cnt into offsets[0 .. rows], and the largest count; tiles, no atomics
//   k_neighbors_fill<P>    the same walk; lane-owned stores indices[offsets[row] + running]
//   k_neighbors_fill_wave<P>   the A/B variant of the fill (SPH_OPT_NEIGHBORS_FILL 1): a wave writes one row at a time, same bits
// Ids are a permutation of [0, n), cellStart ends at n and the fill finds what the count found, so the range guards in these kernels
// (id < n, row < rows, min(cellStart, n), w < end) never fire; they stay so that no load or store can leave its array.
// Candidate rows are read straight from global memory (the LDS-staged scalar sweep lost to the plain walk).
#pragma once
#include <math.h>

#include "sph_query.h"

namespace sph {

constexpr int kNbSelf = 1, kNbHalf = 2, kNbCountOnly = 4;      // SPH_NEIGHBORS_* of sph_abi.h

// Does an entry of a PARTICLE list stay?  own: the candidate is the target's own slot (kept by identity under SELF, never otherwise).
__host__ __device__ inline bool neighbor_keep(int flags, bool own, bool accepted, uint32_t idTarget, uint32_t idCandidate) {
    if (own) return (flags & kNbSelf) != 0;
    return accepted && (!(flags & kNbHalf) || idCandidate > idTarget);
}
// The walk of one target: emit(id of the kept candidate) per entry, in order.  q: the target's own slot (particle lists).
template <bool PARTICLES, class E>
__device__ __forceinline__ void neighbor_walk(const SimK& k, const NbK& nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                              const int32_t* __restrict__ ids, float px, float py, float pz, uint32_t q, uint32_t idTarget, E&& emit) {
    const int3 cell = cell_of(k, px, py, pz);
    const bool half = (nb.flags & kNbHalf) != 0;
    neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
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

template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_neighbors_count(SimK k, NbK nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                            const int32_t* __restrict__ ids, const float4* __restrict__ points, size_t rows,
                                                            uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    size_t row;
    bool walk;
    if (!query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk)) return;
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
    if (!query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk) || !walk) return;
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
    const bool mine = query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk) && walk;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool half = (nb.flags & kNbHalf) != 0;
    for (int t = 0; t < 64; ++t) {                                            // every lane of the wave stays to the end: the targets cross the lanes
        if (!__shfl((int)mine, t, 64)) continue;                             // (wave-uniform)
        const float px = __shfl(P.x, t, 64), py = __shfl(P.y, t, 64), pz = __shfl(P.z, t, 64);
        const uint32_t trow = (uint32_t)__shfl((int)(uint32_t)row, t, 64);   // (rows < 2^31)
        const uint32_t q = (uint32_t)(i0 + (size_t)t);
        long long w = offsets[trow];
        const long long end = offsets[(size_t)trow + 1];
        const int3 cell = cell_of(k, px, py, pz);
        neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
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

}  // namespace sph
