// sph_knn.h -- the k nearest neighbours within a radius, of the particles or of query points (no reference counterpart; DESIGN.md
// section 3m).
//
// Grid, radius rules, stencil, candidates and the target of a lane are those of sph_query.h (neighbor_stencil, neighbor_rows,
// query_target).  A candidate j is accepted when r2 < R2, r2 = knn_r2 (the arithmetic of neighbor_accept), and gets the key
// (bits(r2) << 32) | id_j: r2 is a sum of squares, >= +0 and never -0, so keys compared as uint64 order by ascending r2, ties to the smaller particle id.  The
// row of a target is its min(k, accepted) smallest keys, ascending: one answer whatever the order in which the candidates are met.
// Flags differ from the neighbour lists': without SPH_KNN_SELF the target's own slot is left out by slot identity; WITH it the own
// slot is an ordinary candidate (r2 = 0, ordered by id among coincident particles), so a target with a NaN position keeps an empty
// row (sph_neighbors' SELF keeps such a target by identity).  SPH_KNN_FLUID_ONLY: records with isGhost != 0 (F_GHOSTNZ of the own
// data, as k_components_init reads it) are never candidates and their own rows are empty.
//
//   knn_r2 / knn_key          __host__ __device__: sph_knn_host runs the same functions
//   k_knn<P, KCAP>            the default: one target per lane; the lane's k best keys live in LDS as 8-byte words, [slot][lane], as a
//                             binary max-heap (the worst kept key at slot 0; an accepted key costs at most log2 k levels, where a sorted
//                             row costs up to k shifts and the wave waits for its slowest lane), sorted in place at the end (heap sort).
//                             Word (slot, lane) sits at slot * T + lane with T a multiple of 64, so lane l of a wave is on banks 2l,
//                             2l + 1 (mod 64) WHATEVER its slot: lanes that diverge to different slots still touch distinct banks inside
//                             every lane group of ds_read_b64 / ds_write_b64.  Count and worst kept key stay in registers: a full row
//                             rejects a candidate on one compare of the r2 bits, without touching LDS.
//                             KCAP is 8, 16, 32, 64 (the smallest >= k), with 256, 256, 128, 64 threads: at most 32 KiB of LDS per block.
//   k_knn_select<P>           variant 1 (SPH_OPT_KNN_VARIANT): no LDS, no per-lane storage; pass t of k finds the smallest key above
//                             the one pass t - 1 emitted.  O(k * candidates): the slow second statement of the same bits.
// Both write indices / dist2 padded with (-1, +inf) and counts, and add (sum of counts, rows with count == k) to stats with one
// integer atomic per wave and word.  ids[] is k_neighbors_ids' (a permutation of [0, n)); the range guards (row < rows, j < end <= n,
// slot < KCAP) stay so that no load or store can leave its array.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_query.h"

namespace sph {

constexpr int kKnnSelf = 1, kKnnFluidOnly = 2;      // SPH_KNN_* of sph_abi.h
constexpr int kKnnMaxK = 64;                        // SPH_KNN_MAX_K
constexpr unsigned long long kKnnNoKey = ~0ull;     // above every key: the high word of a key is the bits of a finite r2

// The squared distance of neighbor_accept, returned: dot3 of sph_device.h; NaN on either side gives NaN (accepted by no radius).
__host__ __device__ inline float knn_r2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return dot3(dx, dy, dz, dx, dy, dz);
}
__host__ __device__ inline uint32_t knn_bits(float r2) {
    uint32_t u;
    memcpy(&u, &r2, 4);
    return u;
}
__host__ __device__ inline unsigned long long knn_key(float r2, uint32_t id) { return ((unsigned long long)knn_bits(r2) << 32) | (unsigned long long)id; }
__host__ __device__ inline float knn_key_r2(unsigned long long key) {
    const uint32_t u = (uint32_t)(key >> 32);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// Smallest class 8, 16, 32, 64 that holds k (1 <= k <= 64).
inline int knn_class(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
constexpr int knn_threads(int kcap) { return kcap <= 16 ? 256 : kcap == 32 ? 128 : 64; }

// The walk of one target: f(slot j, r2) per accepted candidate, in slot order.  q: the target's own slot (particle rows).
template <bool PARTICLES, class F>
__device__ __forceinline__ void knn_walk(const SimK& k, const NbK& nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                         float px, float py, float pz, uint32_t q, F&& f) {
    const int3 cell = cell_of(k, px, py, pz);
    const bool skipOwn = PARTICLES && !(nb.flags & kKnnSelf);
    neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            if (skipOwn && j == q) continue;
            const float4 J = pv[2u * j];
            const float r2 = knn_r2(px, py, pz, J.x, J.y, J.z);
            if (r2 < nb.R2) f(j, r2);
        }
    });
}

// Target of a lane (query_target) and whether it walks: a ghost's particle row is empty under FLUID_ONLY.
template <bool PARTICLES>
__device__ __forceinline__ bool knn_target(const NbK& nb, const float4* __restrict__ pv, const int32_t* __restrict__ ids, const float4* __restrict__ own,
                                           const float4* __restrict__ points, size_t rows, size_t i, float4& P, size_t& row, bool& walk) {
    if (!query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk)) return false;
    if (PARTICLES && walk && (nb.flags & kKnnFluidOnly)) walk = !slot_ghost(own, (uint32_t)i);
    return true;
}
// (sum of counts, full rows) of the wave into stats[0], stats[1]: every lane of the wave must arrive.
__device__ __forceinline__ void knn_reduce(uint32_t cnt, bool full, unsigned long long* __restrict__ stats) {
    const uint32_t s = wave_sum(cnt);
    const unsigned long long nf = (unsigned long long)__popcll(__ballot(full));
    if ((threadIdx.x & 63) == 0) {
        if (s) atomicAdd(stats + 0, (unsigned long long)s);
        if (nf) atomicAdd(stats + 1, nf);
    }
}

// Puts `key` into the max-heap of n keys of lane t whose root is vacant: the larger child moves up while it is above the key.  Returns
// what ends up at the root.  T: the stride between the slots of one lane.
template <int T>
__device__ __forceinline__ unsigned long long knn_sift_down(unsigned long long* best, int t, int n, unsigned long long key) {
    int i = 0;
    unsigned long long top = key;
    for (;;) {
        const int l = 2 * i + 1, r = l + 1;
        if (l >= n) break;
        const unsigned long long a = best[l * T + t], b = r < n ? best[r * T + t] : 0ull;
        const bool right = b > a;                                               // (keys of one row are distinct; without a right child: left)
        const unsigned long long c = right ? b : a;
        if (c < key) break;
        best[i * T + t] = c;
        if (i == 0) top = c;
        i = right ? r : l;
    }
    best[i * T + t] = key;
    return top;
}

template <bool PARTICLES, int KCAP>
__global__ __launch_bounds__(knn_threads(KCAP)) void k_knn(SimK k, NbK nb, int kk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                           const int32_t* __restrict__ ids, const float4* __restrict__ own,
                                                           const float4* __restrict__ points, size_t rows, int32_t* __restrict__ indices,
                                                           float* __restrict__ dist2, uint32_t* __restrict__ counts, unsigned long long* __restrict__ stats) {
    constexpr int T = knn_threads(KCAP);
    static_assert(T % 64 == 0 && KCAP * T * 8 <= 32768, "a lane keeps its banks whatever its slot; 32 KiB of LDS per block");
    __shared__ unsigned long long best[KCAP * T];                               // [slot][lane]: a max-heap over the slots below the lane's count
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * T + t;
    const int K = max(1, min(kk, KCAP));
    const bool fluidOnly = (nb.flags & kKnnFluidOnly) != 0;
    float4 P;
    size_t row = 0;
    bool walk = false;
    const bool act = knn_target<PARTICLES>(nb, pv, ids, own, points, rows, i, P, row, walk);
    int cnt = 0;
    unsigned long long worst = kKnnNoKey;                                       // the largest kept key once the row is full; above every key before
    if (act && walk) {
        knn_walk<PARTICLES>(k, nb, pv, cellStart, P.x, P.y, P.z, (uint32_t)i, [&](uint32_t j, float r2) {
            if (knn_bits(r2) > (uint32_t)(worst >> 32)) return;                 // a full row: the one further compare
            if (fluidOnly && slot_ghost(own, j)) return;
            const unsigned long long key = knn_key(r2, (uint32_t)ids[j]);
            if (key >= worst) return;                                           // (equal r2 bits, a larger id)
            if (cnt == K) {                                                     // a full row drops its worst: the root
                worst = knn_sift_down<T>(best, t, K, key);
                return;
            }
            int leaf = cnt;                                                     // a new leaf climbs while its parent is below it
            while (leaf > 0) {
                const int up = (leaf - 1) >> 1;
                const unsigned long long parent = best[up * T + t];
                if (parent > key) break;
                best[leaf * T + t] = parent;
                leaf = up;
            }
            best[leaf * T + t] = key;
            if (++cnt == K) worst = best[t];
        });
    }
    if (act) {
        for (int end = cnt - 1; end > 0; --end) {                               // heap sort: the largest of [0, end] goes to slot end
            const unsigned long long last = best[end * T + t];
            best[end * T + t] = best[t];
            (void)knn_sift_down<T>(best, t, end, last);
        }
        const size_t base = row * (size_t)K;
        for (int s = 0; s < K; ++s) {
            const bool have = s < cnt;
            const unsigned long long key = have ? best[s * T + t] : 0ull;
            indices[base + s] = have ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
            dist2[base + s] = have ? knn_key_r2(key) : INFINITY;
        }
        counts[row] = (uint32_t)cnt;
    }
    knn_reduce(act ? (uint32_t)cnt : 0u, act && cnt == K, stats);
}

template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_knn_select(SimK k, NbK nb, int kk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                       const int32_t* __restrict__ ids, const float4* __restrict__ own,
                                                       const float4* __restrict__ points, size_t rows, int32_t* __restrict__ indices,
                                                       float* __restrict__ dist2, uint32_t* __restrict__ counts, unsigned long long* __restrict__ stats) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const int K = max(1, min(kk, kKnnMaxK));
    const bool fluidOnly = (nb.flags & kKnnFluidOnly) != 0;
    float4 P;
    size_t row = 0;
    bool walk = false;
    const bool act = knn_target<PARTICLES>(nb, pv, ids, own, points, rows, i, P, row, walk);
    int cnt = 0;
    if (act) {
        const size_t base = row * (size_t)K;
        unsigned long long last = 0ull;                                         // the key of the pass before (cnt > 0)
        for (int s = 0; s < K; ++s) {
            unsigned long long found = kKnnNoKey;
            if (walk) {
                knn_walk<PARTICLES>(k, nb, pv, cellStart, P.x, P.y, P.z, (uint32_t)i, [&](uint32_t j, float r2) {
                    if (fluidOnly && slot_ghost(own, j)) return;
                    const unsigned long long key = knn_key(r2, (uint32_t)ids[j]);
                    if ((cnt == 0 || key > last) && key < found) found = key;
                });
            }
            const bool have = found != kKnnNoKey;
            walk = walk && have;                                                // no key above the last one: the row has ended
            indices[base + s] = have ? (int32_t)(uint32_t)(found & 0xffffffffull) : -1;
            dist2[base + s] = have ? knn_key_r2(found) : INFINITY;
            if (have) { last = found; ++cnt; }
        }
        counts[row] = (uint32_t)cnt;
    }
    knn_reduce(act ? (uint32_t)cnt : 0u, act && cnt == K, stats);
}

}  // namespace sph
