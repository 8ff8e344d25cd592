// sph_aggregate.h -- fused neighbourhood reductions of a caller's per-particle tensor: sum, mean, max, min of values[j][0 .. C) over the
// neighbours j of every particle or of query points (no reference counterpart).
//
// Grid, radius rules, stencil, candidate rows and the target of a lane are those of sph_query.h (neighbor_stencil, neighbor_rows,
// query_target); a candidate is accepted by neighbor_offset (d = x_j - x_i, r2 = dot3(d, d) < R2), a particle target's own slot by slot
// identity under SELF (d = 0, r2 = 0 exactly) and never otherwise.  FLUID_ONLY: ghost records are no candidates and a ghost target's row
// is empty.  Every channel has one fp32 accumulator that takes the accepted candidates in slot order; every product and sum is rounded
// on its own (no fmaf: the build's -ffp-contract=off), so the twin that runs the same functions over HostGrid gives the same bytes.
//
//   aggregate_accept / _weight / _value / _add / _add_moment / _extremum / _mean   __host__ __device__: sph_aggregate_host runs them too
//   k_aggregate_stage         xs[slot][c] = x[id][c]: the caller's rows in slot order, so that the payload of a row run is contiguous and
//                             the lanes of a wave (neighbouring slots of one cell) read the same lines
//   k_aggregate<P, X, M, CH>  one target per lane (P: sorted-slot order, rows numbered by id; else the caller's points); X: extremum
//                             (MAX / MIN) instead of the sums; M: the three first-moment planes beside the sum; CH: channels per pass.
//                             A lane keeps planes x CH accumulators in registers and walks its candidates once per chunk of CH channels.
//                             AggK.byId: the payload is gathered from the caller's array through ids[] (SPH_OPT_AGGREGATE_VARIANT bit 0,
//                             no stage); AggK.vec4: 16-byte payload loads (C % 4 == 0 and a 16-byte aligned base).  The same bits all ways.
// Stores are lane-owned, by row; no atomics.  ids[] is k_neighbors_ids' (a permutation of [0, n)), candidate slots end at n and a
// channel index stays below C, so the range guards (row < rows, j < n, c < C) never fire; they stay so that no load or store can
// leave its array.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_query.h"

namespace sph {

constexpr int kAggSelf = 1, kAggFluidOnly = 2, kAggDelta = 4, kAggMoments = 8;      // SPH_AGGREGATE_* flags of sph_abi.h
constexpr int kAggSum = 0, kAggMean = 1, kAggMax = 2, kAggMin = 3;                  // SPH_AGGREGATE_SUM ..
constexpr int kAggWeightOne = 0, kAggWeightPoly6 = 1;                               // SPH_AGGREGATE_WEIGHT_*
constexpr int kAggMaxChannels = 128;                                                // SPH_AGGREGATE_MAX_CHANNELS
// Channels per pass of the walk where SPH_OPT_AGGREGATE_VARIANT does not say: the smallest of 4, 8, 16 that holds C.  Measured at C = 1, 4, 16,
// 64: a chunk wider than C pays for lanes of accumulators nobody stores, a narrower one for further walks.
inline int aggregate_chunk(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : 16; }

struct AggK {
    int op, weight, C;
    int byId, vec4;          // the payload comes from values[ids[j]] (no stage) / in 16-byte loads
};

// float bits -> unsigned order and back: the map of the ray keys (-0 below +0, -inf lowest, +inf highest of the numbers).
__host__ __device__ inline uint32_t agg_ordered(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float agg_unordered(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
constexpr uint32_t kAggLowest = 0x007FFFFFu, kAggHighest = 0xFF800000u;             // agg_ordered(-inf), agg_ordered(+inf)

// Does candidate slot j enter the row of a target at xi?  own: j is the particle target's own slot.
__host__ __device__ inline bool aggregate_accept(bool own, bool self, float xi, float yi, float zi, float xj, float yj, float zj, float R2,
                                                 float& dx, float& dy, float& dz, float& r2) {
    if (own) {
        dx = dy = dz = r2 = 0.0f;
        return self;
    }
    return neighbor_offset(xi, yi, zi, xj, yj, zj, R2, dx, dy, dz, r2);
}
__host__ __device__ inline float aggregate_weight(int weight, float R2, float r2) {
    if (weight == kAggWeightOne) return 1.0f;
    const float t = R2 - r2;
    return (t * t) * t;
}
__host__ __device__ inline float aggregate_value(bool delta, float vj, float vi) { return delta ? vj - vi : vj; }
__host__ __device__ inline float aggregate_add(float acc, float w, float v) { return acc + w * v; }
__host__ __device__ inline float aggregate_add_moment(float acc, float w, float d, float v) { return acc + (w * d) * v; }
// The best ordered key so far (MAX: the largest, from kAggLowest; MIN: the smallest, from kAggHighest); a NaN never wins.
__host__ __device__ inline uint32_t aggregate_extremum(bool isMax, uint32_t best, float v) {
    if (v != v) return best;
    const uint32_t key = agg_ordered(v);
    return (isMax ? key > best : key < best) ? key : best;
}
__host__ __device__ inline float aggregate_mean(float acc, float W) { return W == 0.0f ? 0.0f : acc / W; }

__global__ __launch_bounds__(kBlock) void k_aggregate_stage(const int32_t* __restrict__ ids, const float* __restrict__ x, float* __restrict__ xs, uint32_t n, int C) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)n * (size_t)C) return;
    const size_t slot = t / (size_t)C, c = t - slot * (size_t)C;
    const uint32_t id = (uint32_t)ids[slot];
    if (id < n) xs[t] = x[(size_t)id * (size_t)C + c];
}

template <bool PARTICLES, bool EXTREMUM, bool MOMENTS, int CH>
__global__ __launch_bounds__(kBlock) void k_aggregate(SimK k, NbK nb, AggK ag, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                      const int32_t* __restrict__ ids, const float4* __restrict__ own, const float4* __restrict__ points,
                                                      size_t rows, const float* __restrict__ vals, float* __restrict__ out, uint32_t* __restrict__ count) {
    static_assert(!(EXTREMUM && MOMENTS) && CH % 4 == 0, "moments go with the sum; a chunk is whole 16-byte groups");
    constexpr int PLANES = MOMENTS ? 4 : 1;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    size_t row;
    bool walk;
    if (!query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk)) return;
    const bool self = (nb.flags & kAggSelf) != 0, fluidOnly = (nb.flags & kAggFluidOnly) != 0, delta = PARTICLES && (nb.flags & kAggDelta) != 0;
    const bool isMax = ag.op == kAggMax;
    if (PARTICLES && fluidOnly && slot_ghost(own, (uint32_t)i)) walk = false;
    const uint32_t q = (uint32_t)i;
    const int C = ag.C;
    const size_t mineAt = (ag.byId ? row : i) * (size_t)C;                      // the target's own values (DELTA)
    float* __restrict__ orow = out + row * (size_t)(PLANES * C);
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    for (int c0 = 0; c0 < C; c0 += CH) {
        float acc[PLANES][CH], mine[CH], W = 0.0f;
        uint32_t best[CH], cnt = 0u;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
#pragma unroll
            for (int p = 0; p < PLANES; ++p) acc[p][u] = 0.0f;
            best[u] = isMax ? kAggLowest : kAggHighest;
            mine[u] = (delta && c0 + u < C) ? vals[mineAt + (size_t)(c0 + u)] : 0.0f;
        }
        if (walk) {
            neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    const float4 J = pv[2u * j];
                    float dx, dy, dz, r2;
                    if (!aggregate_accept(PARTICLES && j == q, self, P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && slot_ghost(own, j)) continue;
                    const uint32_t src = ag.byId ? (uint32_t)ids[j] : j;
                    const float* __restrict__ vrow = vals + (size_t)src * (size_t)C + (size_t)c0;
                    float v[CH];
                    if (ag.vec4) {
#pragma unroll
                        for (int g = 0; g < CH; g += 4) {
                            const float4 t = (c0 + g < C) ? *reinterpret_cast<const float4*>(vrow + g) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                            v[g] = t.x; v[g + 1] = t.y; v[g + 2] = t.z; v[g + 3] = t.w;
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < CH; ++u) v[u] = (c0 + u < C) ? vrow[u] : 0.0f;
                    }
                    const float w = aggregate_weight(ag.weight, nb.R2, r2);
                    cnt += 1u;
                    W = W + w;
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        const float val = aggregate_value(delta, v[u], mine[u]);
                        if (EXTREMUM) {
                            best[u] = aggregate_extremum(isMax, best[u], val);
                        } else {
                            acc[0][u] = aggregate_add(acc[0][u], w, val);
                            if (MOMENTS) {
                                acc[PLANES - 3][u] = aggregate_add_moment(acc[PLANES - 3][u], w, dx, val);
                                acc[PLANES - 2][u] = aggregate_add_moment(acc[PLANES - 2][u], w, dy, val);
                                acc[PLANES - 1][u] = aggregate_add_moment(acc[PLANES - 1][u], w, dz, val);
                            }
                        }
                    }
                }
            });
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (c0 + u >= C) continue;
            if (EXTREMUM) {
                orow[c0 + u] = agg_unordered(best[u]);
            } else {
#pragma unroll
                for (int p = 0; p < PLANES; ++p) orow[p * C + c0 + u] = (p == 0 && ag.op == kAggMean) ? aggregate_mean(acc[0][u], W) : acc[p][u];
            }
        }
        if (c0 == 0 && count) count[row] = cnt;
    }
}

}  // namespace sph
