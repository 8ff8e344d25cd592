// sph_components.h -- connected components of the neighbour relation (bodies of fluid, droplets) with a table per body (no reference
// counterpart).
//
// The graph: records i != j are joined when j is a candidate of i (sph_query.h: the cells [c - s, c + s] per axis) and
// neighbor_accept holds.  The relation is symmetric bit for bit, so its components are a well-defined result; they are named by the
// smallest particle id they hold, which makes the output independent of the order in which anything below happens.
//
// Everything works on sorted slots: parent[q] is a slot, a slot's candidates are slots nearby in memory, pv[2 q] its position.
//
//   k_components_init      parent[q] = q, minId[q] = none, ids[q] = particle id of the slot (~id for a record that does not take part)
//   k_components_hook      one target per lane over the walk of k_neighbors_count; per accepted candidate j < q (an edge is seen from
//                          its larger end, half the loads): the roots of q and j by chasing parent; if they differ,
//                          atomicMin(parent[larger root], smaller root) and the launch's "changed" word is set
//   k_components_compress  parent[q] <- an ancestor up to kCcHops hops up; a launch of its own, so that no plain store meets a hook's
//                          atomic; repeated until a launch finds every slot below a root (its "more" word stays 0)
//   The host repeats hook + compress until a WHOLE hook launch has found every edge inside one tree: that launch wrote nothing, so what
//   it read was final.  This criterion, not an ordering argument, is what makes the result right under races and under stale reads.
//   Invariants (every store to parent keeps them):
//     1. parent[x] <= x always, and parent[x] == x exactly for a root;
//     2. a value is only ever lowered, and only to a slot of the same component of the graph (a stale read is an older such value:
//        it can cost a round, never join two bodies);
//     3. no lane waits for another lane: no spin, no lock, no retry.  Every chase descends strictly (fewer than n hops), every loop
//        over launches has a cap on the host (kCcMaxRounds hook launches, kCcMaxJumps compress launches per round).
//   Nothing relies on one workgroup seeing another's stores inside a launch; between launches the stream orders them.
//
//   k_components_minid     minId[root slot] = smallest particle id of the tree: equal roots combine across the wave first, one atomicMin
//   k_components_roots     roots[id] = that id (or -1), flag[id] = (roots[id] == id); the k_neighbors_scan_* kernels number the flags
//   k_components_table_init / _label / _finish   labels[id], and the table: count, fixed-point position sums, the box as ordered integers;
//                          lanes of a wave that hold the same label combine across the wave (a match on the leader's label, repeated
//                          until every lane is served), the leader issues the integer atomics.  All integer: exact in any order.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_query.h"

namespace sph {

constexpr int kCcFluidOnly = 1;                  // SPH_COMPONENTS_FLUID_ONLY of sph_abi.h
constexpr uint32_t kCcNonFinite = 1u;            // SPH_COMPONENT_NONFINITE
constexpr int kCcMaxRounds = 64;                 // hook launches of a build
constexpr int kCcMaxJumps = 64;                  // compress launches behind one hook launch
constexpr int kCcHops = 16;                      // ancestors a lane climbs per compress launch
constexpr int kCcWords = kCcMaxRounds * (kCcMaxJumps + 1);   // one "changed" / "more" word per launch, zeroed once per build
constexpr uint32_t kCcNone = 0xffffffffu;
constexpr int kCcFullWalk = 1, kCcLaneAtomics = 2;            // SPH_OPT_COMPONENTS_VARIANT bits (timing A/B, same bits)

// SphComponent of sph_abi.h as the kernels accumulate it: the box as ordered integers until k_components_finish decodes it in place.
struct CcRow {
    uint32_t root, count;
    uint32_t bbMin[3], bbMax[3];
    unsigned long long sumQ[3];
    uint32_t flags, pad;
};
static_assert(sizeof(CcRow) == 64, "CcRow is SphComponent: 64 bytes");

// fp32 <-> an unsigned integer with the same order (-0 below +0; NaN never gets here).
__host__ __device__ inline uint32_t cc_ordered(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float cc_unordered(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// One axis of the fixed-point position: subtract, multiply (each rounded in fp64), clamp to +-2^36, round to nearest even.
__host__ __device__ inline long long cc_fixed(float x, float gmin, double S) {
    const double d = ((double)x - (double)gmin) * S;
    return llrint(fmin(fmax(d, -68719476736.0), 68719476736.0));
}
__host__ __device__ inline bool cc_finite3(float x, float y, float z) { return float_finite(x) && float_finite(y) && float_finite(z); }

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above slot x as far as this lane can see it.  parent[x] < x below a root, so the loop ends after fewer than n hops.
__device__ __forceinline__ uint32_t cc_find(const uint32_t* parent, uint32_t x, uint32_t n) {
    for (uint32_t hop = 0; hop < n; ++hop) {
        const uint32_t p = cc_load(parent + x);
        if (p >= x) break;
        x = p;
    }
    return x;
}

// One lane of the wave sets *word if any lane asks for it.  Every lane of the wave must arrive.
__device__ __forceinline__ void cc_raise(bool ask, uint32_t* word) {
    const unsigned long long any = __ballot(ask);
    if (any && (int)(threadIdx.x & 63) == __ffsll((long long)any) - 1) __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// f(key, mine, leader) once per distinct key among the active lanes: `mine` marks the lanes that hold it, `leader` is the first of
// them.  At most 64 turns (each serves its leader).  Every lane of the wave must arrive.
template <class F>
__device__ __forceinline__ void cc_for_each_key(uint32_t key, bool active, F&& f) {
    unsigned long long todo = __ballot(active);
    for (int turn = 0; turn < 64 && todo; ++turn) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader, 64);
        const bool mine = active && key == lk;
        f(lk, mine, leader);
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(kBlock) void k_components_init(const float4* __restrict__ own, int32_t* __restrict__ ids, uint32_t* __restrict__ parent,
                                                            uint32_t* __restrict__ minId, uint32_t idBase, uint32_t n, int flags) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const float4 o = own[q];
    uint32_t id = fbits(o.w) - idBase;
    if (id >= n) id = 0u;                                                           // (never: ids are idBase + [0, n))
    const bool out = (flags & kCcFluidOnly) && (fbits(o.z) & F_GHOSTNZ);
    ids[q] = out ? ~(int32_t)id : (int32_t)id;
    parent[q] = q;
    minId[q] = kCcNone;
}

// HALF: candidates j < q only.  The full walk sees every edge from both ends and does the same hooks (the A/B of DESIGN.md section 6).
template <bool HALF>
__global__ __launch_bounds__(kBlock) void k_components_hook(SimK k, NbK nb, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                            const int32_t* __restrict__ ids, uint32_t* parent, uint32_t* changed) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool fluidOnly = (nb.flags & kCcFluidOnly) != 0;
    const bool act = q < nb.n && !(fluidOnly && ids[q] < 0);
    bool hooked = false;
    if (act) {
        const float4 P = pv[2u * q];
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        uint32_t rq = kCcNone;                                                      // an ancestor of q (or q), read on the first accepted candidate
        neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
            const uint32_t end = HALF ? min(qe, q) : qe;
            for (uint32_t j = qs; j < end; ++j) {
                if (!HALF && j == q) continue;
                const float4 J = pv[2u * j];
                if (!neighbor_accept(P.x, P.y, P.z, J.x, J.y, J.z, nb.R2)) continue;
                if (fluidOnly && ids[j] < 0) continue;
                if (rq == kCcNone) rq = cc_load(parent + q);
                const uint32_t pj = cc_load(parent + j);
                if (pj == rq) continue;                                             // a common ancestor: the edge is inside one tree
                rq = cc_find(parent, rq, nb.n);
                const uint32_t rj = cc_find(parent, pj, nb.n);
                if (rq == rj) continue;
                const uint32_t hi = max(rq, rj), lo = min(rq, rj);                  // lo < hi < n
                atomicMin(parent + hi, lo);                                         // (agent scope; invariants 1 and 2)
                rq = lo;                                                            // in q's component whoever won at parent[hi]
                hooked = true;
            }
        });
    }
    cc_raise(hooked, changed);
}

__global__ __launch_bounds__(kBlock) void k_components_compress(uint32_t* parent, uint32_t n, uint32_t* more) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    bool unfinished = false;
    if (q < n) {
        const uint32_t p = parent[q];                                               // p <= q < n
        uint32_t x = p;
        for (int hop = 0; hop < kCcHops; ++hop) {
            const uint32_t g = parent[x];
            if (g >= x) break;
            x = g;
        }
        unfinished = parent[x] < x;                                                 // roots do not change in this launch: x == parent[x] is final
        if (x != p) parent[q] = x;
    }
    cc_raise(unfinished, more);
}

__global__ __launch_bounds__(kBlock) void k_components_minid(const int32_t* __restrict__ ids, const uint32_t* __restrict__ parent,
                                                             uint32_t* __restrict__ minId, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const int32_t v = q < n ? ids[q] : -1;
    const bool act = v >= 0;
    const uint32_t root = act ? min(parent[q], n - 1u) : 0u;
    const int lane = threadIdx.x & 63;
    cc_for_each_key(root, act, [&](uint32_t slot, bool mine, int leader) {
        const uint32_t m = wave_min(mine ? (uint32_t)v : kCcNone);
        if (lane == leader) atomicMin(minId + slot, m);
    });
}

__global__ __launch_bounds__(kBlock) void k_components_roots(const int32_t* __restrict__ ids, const uint32_t* __restrict__ parent,
                                                             const uint32_t* __restrict__ minId, int32_t* __restrict__ roots,
                                                             uint32_t* __restrict__ flag, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const int32_t v = ids[q];
    const uint32_t id = v >= 0 ? (uint32_t)v : (uint32_t)~v;
    if (id >= n) return;                                                            // (never)
    const uint32_t r = v >= 0 ? minId[min(parent[q], n - 1u)] : kCcNone;
    roots[id] = v >= 0 ? (int32_t)r : -1;
    flag[id] = (v >= 0 && r == id) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_components_table_init(CcRow* __restrict__ table, uint32_t rows) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= rows) return;
    CcRow r;
    r.root = 0u; r.count = 0u;
    for (int a = 0; a < 3; ++a) { r.bbMin[a] = 0xffffffffu; r.bbMax[a] = 0u; r.sumQ[a] = 0ull; }
    r.flags = 0u; r.pad = 0u;
    table[c] = r;
}

// AGG: equal labels combine across the wave before one lane touches memory; else every lane issues its own atomics (the A/B).
template <bool AGG>
__global__ __launch_bounds__(kBlock) void k_components_label(SimK k, double S, const float4* __restrict__ pv, const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ roots, const long long* __restrict__ offsets,
                                                             int32_t* __restrict__ labels, CcRow* __restrict__ table, uint32_t n, uint32_t rows) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t v = q < n ? ids[q] : -1;
    uint32_t id = v >= 0 ? (uint32_t)v : (uint32_t)~v;
    bool act = false, fin = false;
    uint32_t lab = 0u;
    unsigned long long sq[3] = {0ull, 0ull, 0ull};
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (q < n && id < n) {
        if (v < 0) {
            labels[id] = -1;
        } else {
            const uint32_t r = (uint32_t)roots[id];
            lab = r < n ? (uint32_t)offsets[r] : rows;
            act = lab < rows;                                                       // (always)
            if (act) {
                labels[id] = (int32_t)lab;
                const float4 P = pv[2u * q];
                fin = cc_finite3(P.x, P.y, P.z);
                if (r == id) atomicMax(&table[lab].root, id);                       // one lane per row (an atomic like every access to the row here)
                if (!fin) atomicOr(&table[lab].flags, kCcNonFinite);                // (a body of one)
                if (fin) {
                    const float x[3] = {P.x, P.y, P.z}, g[3] = {k.gminx, k.gminy, k.gminz};
                    for (int a = 0; a < 3; ++a) {
                        sq[a] = (unsigned long long)cc_fixed(x[a], g[a], S);
                        lo[a] = hi[a] = cc_ordered(x[a]);
                    }
                }
            }
        }
    }
    if (AGG) {
        cc_for_each_key(lab, act, [&](uint32_t row, bool mine, int leader) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
            const bool any = __ballot(mine && fin) != 0ull;                         // (wave-uniform)
            unsigned long long s[3] = {0ull, 0ull, 0ull};
            uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
            if (any) {
                for (int a = 0; a < 3; ++a) {
                    s[a] = wave_sum(mine ? sq[a] : 0ull);
                    mn[a] = wave_min(mine ? lo[a] : 0xffffffffu);
                    mx[a] = wave_max(mine ? hi[a] : 0u);
                }
            }
            if (lane == leader) {
                CcRow* t = table + row;
                atomicAdd(&t->count, cnt);
                if (any)
                    for (int a = 0; a < 3; ++a) {
                        atomicAdd(&t->sumQ[a], s[a]);
                        atomicMin(&t->bbMin[a], mn[a]);
                        atomicMax(&t->bbMax[a], mx[a]);
                    }
            }
        });
    } else if (act) {
        CcRow* t = table + lab;
        atomicAdd(&t->count, 1u);
        if (fin)
            for (int a = 0; a < 3; ++a) {
                atomicAdd(&t->sumQ[a], sq[a]);
                atomicMin(&t->bbMin[a], lo[a]);
                atomicMax(&t->bbMax[a], hi[a]);
            }
    }
}

// Decodes the boxes in place and reduces the table: stats[0] = max over rows of (count << 32 | ~root) (the largest body, ties to the
// smaller root), stats[1] = rows with count 1, stats[2] = the sum of the counts.  One block reduction, then one integer atomic per
// block and word.
__global__ __launch_bounds__(kBlock) void k_components_finish(CcRow* __restrict__ table, uint32_t rows, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long sm[3][4];
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long key = 0ull, ones = 0ull, total = 0ull;
    if (c < rows) {
        CcRow r = table[c];
        const bool empty = (r.flags & kCcNonFinite) || r.count == 0u || r.bbMin[0] > r.bbMax[0];
        for (int a = 0; a < 3; ++a) {
            const float mn = empty ? 0.0f : cc_unordered(r.bbMin[a]), mx = empty ? 0.0f : cc_unordered(r.bbMax[a]);
            r.bbMin[a] = fbits(mn);
            r.bbMax[a] = fbits(mx);
        }
        table[c] = r;
        key = ((unsigned long long)r.count << 32) | (unsigned long long)(~r.root);
        ones = r.count == 1u ? 1ull : 0ull;
        total = r.count;
    }
    key = wave_max(key);
    ones = wave_sum(ones);
    total = wave_sum(total);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sm[0][w] = key; sm[1][w] = ones; sm[2][w] = total; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long kmax = sm[0][0];
        for (int i = 1; i < 4; ++i) kmax = sm[0][i] > kmax ? sm[0][i] : kmax;
        atomicMax(stats + 0, kmax);
        atomicAdd(stats + 1, sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3]);
        atomicAdd(stats + 2, sm[2][0] + sm[2][1] + sm[2][2] + sm[2][3]);
    }
}

}  // namespace sph
