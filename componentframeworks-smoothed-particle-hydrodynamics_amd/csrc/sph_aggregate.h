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
#define SPH_AGGREGATE_H 1     // (sph_conv.h, which is built on this header, checks that it came first)
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

// ---- the adjoint of SUM: out[k][c] = sum over the rows i that accept k ----------------------------------------
// Row i's offset to candidate k is d = x_k - x_i: the walk of particle k hands its candidates to aggregate_accept as the TARGET and
// itself as the candidate, so d, r2 and w are the forward's bits.  The box stencil is symmetric (|c_i - c_k| <= s per axis both ways,
// with clamped cells on both sides), so "row i's cell lies in my stencil" is "my cell lies in row i's stencil": the rows found are
// exactly the rows that accept k, in ascending sorted slot (particle targets) or ascending (clamped cell, point index) (query targets).
//   aggregate_adjoint_plane0 / _moment   __host__ __device__ per-term values: sph_aggregate_adjoint_host runs them too
//   k_adjoint_bin / _scatter / _rank     counting sort of the finite query points by clamped cell (the engine's scan in between); the
//                                        atomic's arrival order is removed by k_adjoint_rank: ascending point index inside a cell
//   k_adjoint_stage                      dst[slot][.] = src[perm[slot]][.] in 4-byte words: the rows of g (and of arg) in row order
//   k_aggregate_adjoint<Q, M, D, CH>     one particle per lane in sorted-slot order; Q: the rows are binned query points, else sorted
//                                        slots; M: g has the three moment planes; D: DELTA.  Particle targets without MOMENTS never come
//                                        here: their adjoint is the forward of g (the relation and the weights are symmetric).
//   k_aggregate_route<Q, CH>             the same walk; out[k][c] = the sum of g[i][c] over the rows with arg[i][c] == k, acc = acc + g
// and the extrema that say who won:
//   aggregate_arg_step                   __host__ __device__: the best key and the smallest id that holds it
//   k_aggregate_arg<P, CH>               k_aggregate's extremum walk with the winner's id beside the key
__host__ __device__ inline float aggregate_adjoint_plane0(bool delta, float gi, float gk) { return delta ? gi - gk : gi; }
__host__ __device__ inline float aggregate_adjoint_moment(bool delta, float gi, float gk) { return delta ? gi + gk : gi; }
// aggregate_extremum with the winner: arg is the smallest id among the non-NaN values whose key is the best one (kAggNoArg: none yet).
// The first value whose key equals the start key (-inf for MAX, +inf for MIN) wins by the equality branch.
constexpr uint32_t kAggNoArg = 0xFFFFFFFFu;
__host__ __device__ inline void aggregate_arg_step(bool isMax, uint32_t& best, uint32_t& arg, float v, uint32_t id) {
    if (v != v) return;
    const uint32_t key = agg_ordered(v);
    if (isMax ? key > best : key < best) { best = key; arg = id; }
    else if (key == best && id < arg) arg = id;
}

constexpr uint32_t kAdjNoCell = 0xFFFFFFFFu;           // the key of a point with a non-finite coordinate: it is not binned

__global__ __launch_bounds__(kBlock) void k_adjoint_bin(SimK k, const float4* __restrict__ points, uint2* __restrict__ key, uint32_t* __restrict__ cellCount, uint32_t m) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 p = points[i];
    if (!sample_finite(p.x, p.y, p.z)) { key[i] = make_uint2(kAdjNoCell, 0u); return; }
    const int3 c = cell_of(k, p.x, p.y, p.z);
    const uint32_t cell = (uint32_t)((c.z * k.gy + c.y) * k.gx + c.x);
    key[i] = make_uint2(cell, cell < (uint32_t)k.numCells ? atomicAdd(&cellCount[cell], 1u) : 0u);
}

__global__ __launch_bounds__(kBlock) void k_adjoint_scatter(const uint2* __restrict__ key, const uint32_t* __restrict__ start, uint32_t* __restrict__ tmp, uint32_t m, uint32_t numCells) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint2 q = key[i];
    if (q.x >= numCells) return;
    const uint32_t s = start[q.x] + q.y;
    if (s < m) tmp[s] = i;
}

// perm[start[cell] + rank] = i, rank = the members of i's cell with a smaller index; pts[] the points in that order.
__global__ __launch_bounds__(kBlock) void k_adjoint_rank(const uint2* __restrict__ key, const uint32_t* __restrict__ start, const uint32_t* __restrict__ tmp,
                                                         const float4* __restrict__ points, uint32_t* __restrict__ perm, float4* __restrict__ pts, uint32_t m,
                                                         uint32_t numCells) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t cell = key[i].x;
    if (cell >= numCells) return;
    const uint32_t s = start[cell], e = min(start[cell + 1], m);
    uint32_t rank = 0u;
    for (uint32_t q = s; q < e; ++q) rank += tmp[q] < i ? 1u : 0u;
    if (s + rank < m) { perm[s + rank] = i; pts[s + rank] = points[i]; }
}

// PC words per row; the first min(*binned, m) slots hold a row (binned null: all m; for query rows start[numCells], the finite points).
__global__ __launch_bounds__(kBlock) void k_adjoint_stage(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ binned, const uint32_t* __restrict__ src,
                                                          uint32_t* __restrict__ dst, uint32_t m, int PC) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t mb = binned ? (size_t)min(*binned, m) : (size_t)m;
    if (t >= mb * (size_t)PC) return;
    const size_t slot = t / (size_t)PC, c = t - slot * (size_t)PC;
    const uint32_t from = perm[slot];
    if (from < m) dst[t] = src[(size_t)from * (size_t)PC + c];
}

// What the adjoint kernels know about the rows: positions (every STRIDE-th float4: 2 in the sorted copy, 1 for binned points), the cell
// table of the rows and the bound of a row index (n, or m: never below start[numCells]).
struct AdjRows {
    const float4* __restrict__ pos;
    const uint32_t* __restrict__ start;
    uint32_t end;
};

// The rows that accept the particle in sorted slot q at P, ascending: f(row index, dx, dy, dz, r2) with the forward's d = P - x_row.
template <bool QUERY, class F>
__device__ __forceinline__ void adjoint_walk(const SimK& k, const NbK& nb, const AdjRows& rows, const float4* __restrict__ own, const float4& P, uint32_t q, F&& f) {
    constexpr uint32_t STRIDE = QUERY ? 1u : 2u;
    const bool self = !QUERY && (nb.flags & kAggSelf) != 0, fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    if (fluidOnly && slot_ghost(own, q)) return;                                // a ghost under FLUID_ONLY is nobody's candidate
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    neighbor_rows(k, rows.start, nb.s, rows.end, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            const float4 X = rows.pos[STRIDE * j];
            float dx, dy, dz, r2;
            if (!aggregate_accept(!QUERY && j == q, self, X.x, X.y, X.z, P.x, P.y, P.z, nb.R2, dx, dy, dz, r2)) continue;
            if (!QUERY && fluidOnly && slot_ghost(own, j)) continue;            // a ghost target's row is empty
            f(j, dx, dy, dz, r2);
        }
    });
}

// The particle of a lane: sorted slot q -> (position, id); false: the lane has no particle.
__device__ __forceinline__ bool adjoint_particle(const NbK& nb, const float4* __restrict__ pv, const int32_t* __restrict__ ids, uint32_t q, float4& P, uint32_t& id) {
    if (q >= nb.n) return false;
    P = pv[2u * q];
    id = (uint32_t)ids[q];
    return id < nb.n;
}

// gs: g in row order, [row][planes][C]; out: [n][C] by particle id.
template <bool QUERY, bool MOMENTS, bool DELTA, int CH>
__global__ __launch_bounds__(kBlock) void k_aggregate_adjoint(SimK k, NbK nb, AggK ag, const float4* __restrict__ pv, const int32_t* __restrict__ ids,
                                                              const float4* __restrict__ own, AdjRows rows, const float* __restrict__ gs, float* __restrict__ out) {
    static_assert(!(QUERY && DELTA), "DELTA applies to particle targets only");
    constexpr int PLANES = MOMENTS ? 4 : 1, MINE = DELTA ? PLANES : 1;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    uint32_t id;
    if (!adjoint_particle(nb, pv, ids, q, P, id)) return;
    const int C = ag.C;
    const size_t rowWords = (size_t)(PLANES * C);
    float* __restrict__ orow = out + (size_t)id * (size_t)C;
    for (int c0 = 0; c0 < C; c0 += CH) {
        float acc[CH], mine[MINE][CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            acc[u] = 0.0f;
#pragma unroll
            for (int p = 0; p < MINE; ++p) mine[p][u] = (DELTA && c0 + u < C) ? gs[(size_t)q * rowWords + (size_t)(p * C + c0 + u)] : 0.0f;
        }
        adjoint_walk<QUERY>(k, nb, rows, own, P, q, [&](uint32_t j, float dx, float dy, float dz, float r2) {
            const float* __restrict__ grow = gs + (size_t)j * rowWords + (size_t)c0;
            const float w = aggregate_weight(ag.weight, nb.R2, r2);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                if (c0 + u >= C) continue;
                acc[u] = aggregate_add(acc[u], w, aggregate_adjoint_plane0(DELTA, grow[u], mine[0][u]));
                if (MOMENTS) {
                    acc[u] = aggregate_add_moment(acc[u], w, dx, aggregate_adjoint_moment(DELTA, grow[C + u], mine[MINE > 1 ? 1 : 0][u]));
                    acc[u] = aggregate_add_moment(acc[u], w, dy, aggregate_adjoint_moment(DELTA, grow[2 * C + u], mine[MINE > 1 ? 2 : 0][u]));
                    acc[u] = aggregate_add_moment(acc[u], w, dz, aggregate_adjoint_moment(DELTA, grow[3 * C + u], mine[MINE > 1 ? 3 : 0][u]));
                }
            }
        });
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (c0 + u < C) orow[c0 + u] = acc[u];
    }
}

// args / gs: arg and g in row order, [row][C].
template <bool QUERY, int CH>
__global__ __launch_bounds__(kBlock) void k_aggregate_route(SimK k, NbK nb, AggK ag, const float4* __restrict__ pv, const int32_t* __restrict__ ids,
                                                            const float4* __restrict__ own, AdjRows rows, const int32_t* __restrict__ args,
                                                            const float* __restrict__ gs, float* __restrict__ out) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    float4 P;
    uint32_t id;
    if (!adjoint_particle(nb, pv, ids, q, P, id)) return;
    const int C = ag.C;
    float* __restrict__ orow = out + (size_t)id * (size_t)C;
    for (int c0 = 0; c0 < C; c0 += CH) {
        float acc[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) acc[u] = 0.0f;
        adjoint_walk<QUERY>(k, nb, rows, own, P, q, [&](uint32_t j, float, float, float, float) {
            const size_t at = (size_t)j * (size_t)C + (size_t)c0;
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if (c0 + u < C && args[at + u] == (int32_t)id) acc[u] = acc[u] + gs[at + u];
        });
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (c0 + u < C) orow[c0 + u] = acc[u];
    }
}

// k_aggregate<P, true, false, CH> with the winner: vals in slot order; arg[row][C] the smallest id that holds the winning key, or -1.
template <bool PARTICLES, int CH>
__global__ __launch_bounds__(kBlock) void k_aggregate_arg(SimK k, NbK nb, AggK ag, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                          const int32_t* __restrict__ ids, const float4* __restrict__ own, const float4* __restrict__ points,
                                                          size_t rows, const float* __restrict__ vals, float* __restrict__ out, uint32_t* __restrict__ count,
                                                          int32_t* __restrict__ arg) {
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
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    for (int c0 = 0; c0 < C; c0 += CH) {
        float mine[CH];
        uint32_t best[CH], who[CH], cnt = 0u;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            best[u] = isMax ? kAggLowest : kAggHighest;
            who[u] = kAggNoArg;
            mine[u] = (delta && c0 + u < C) ? vals[i * (size_t)C + (size_t)(c0 + u)] : 0.0f;
        }
        if (walk) {
            neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    const float4 J = pv[2u * j];
                    float dx, dy, dz, r2;
                    if (!aggregate_accept(PARTICLES && j == q, self, P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && slot_ghost(own, j)) continue;
                    const float* __restrict__ vrow = vals + (size_t)j * (size_t)C + (size_t)c0;
                    const uint32_t jid = (uint32_t)ids[j];
                    cnt += 1u;
#pragma unroll
                    for (int u = 0; u < CH; ++u)
                        if (c0 + u < C) aggregate_arg_step(isMax, best[u], who[u], aggregate_value(delta, vrow[u], mine[u]), jid);
                }
            });
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (c0 + u >= C) continue;
            out[row * (size_t)C + (size_t)(c0 + u)] = agg_unordered(best[u]);
            arg[row * (size_t)C + (size_t)(c0 + u)] = who[u] == kAggNoArg ? -1 : (int32_t)who[u];
        }
        if (c0 == 0 && count) count[row] = cnt;
    }
}

// The rows of the adjoint on the host: start[] the cell table, order[slot] the row (particle id, or point index) in that slot.  Particle
// rows are HostGrid's; query rows the counting sort of the finite points by clamped cell, ascending index inside a cell.
struct AdjHostRows {
    std::vector<uint32_t> start, order;
    explicit AdjHostRows(const HostGrid& grid) : start(grid.start), order(grid.order) {}
    AdjHostRows(const SimK& k, const float* points4, size_t m) : start((size_t)k.numCells + 1, 0u) {
        std::vector<uint32_t> cellOf(m, kAdjNoCell);
        size_t kept = 0;
        for (size_t i = 0; i < m; ++i) {
            const float* x = points4 + 4 * i;
            if (!(float_finite(x[0]) && float_finite(x[1]) && float_finite(x[2]))) continue;
            const int3 c = cell_of(k, x[0], x[1], x[2]);
            cellOf[i] = (uint32_t)((c.z * k.gy + c.y) * k.gx + c.x);
            start[cellOf[i] + 1] += 1u;
            kept += 1;
        }
        for (size_t c = 0; c < (size_t)k.numCells; ++c) start[c + 1] += start[c];
        order.resize(kept);
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < m; ++i)
            if (cellOf[i] != kAdjNoCell) order[fill[cellOf[i]]++] = (uint32_t)i;
    }
};

// adjoint_walk's twin for particle r: f(row, dx, dy, dz, r2) per row that accepts r, in the rows' order (points4 null: particle rows).
template <class F>
void adjoint_walk_host(const SimK& k, int stencil, const AdjHostRows& rows, const SphParticle* particles, const float* points4, size_t r, float R2, bool self,
                       bool fluidOnly, F&& f) {
    const bool query = points4 != nullptr;
    const float* P = particles[r].pos;
    if (fluidOnly && particles[r].isGhost != 0) return;
    const int3 cell = cell_of(k, P[0], P[1], P[2]);
    neighbor_rows(k, rows.start.data(), stencil, (uint32_t)rows.order.size(), cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            const size_t row = rows.order[j];
            const float* x = query ? points4 + 4 * row : particles[row].pos;
            float dx, dy, dz, r2;
            if (!aggregate_accept(!query && row == r, !query && self, x[0], x[1], x[2], P[0], P[1], P[2], R2, dx, dy, dz, r2)) continue;
            if (!query && fluidOnly && particles[row].isGhost != 0) continue;
            f(row, dx, dy, dz, r2);
        }
    });
}

}  // namespace sph
