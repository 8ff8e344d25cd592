// sph_conv.h -- filter-grid basis sums of a caller's per-particle tensor: A[i][b][c] = sum_j w(r_ij) phi_b(x_j - x_i) x[j][c] over the
// neighbours j of every particle or of query points, phi_b the B = K^3 trilinear hat functions of a K x K x K filter grid laid over
// [-R, R]^3 (the linear part of a continuous convolution; no reference counterpart), and the exact transpose.
// Feature layer above sph_aggregate.h: grid, radius rules, stencil, candidate order, acceptance (aggregate_accept), SELF, FLUID_ONLY,
// weights (aggregate_weight), the staged payload (k_aggregate_stage), the point binning (k_adjoint_bin / _scatter / _rank) and the row
// tables of the transposed walk (AdjRows) are that header's.  Every product and sum is rounded on its own (no fmaf: the build's
// -ffp-contract=off).
//
//   basis_axis / basis_corners / basis_add   __host__ __device__: the twins sph_aggregate_basis_host / _adjoint_host run them too
//   k_aggregate_basis<P>          a group of G = 4 .. 64 lanes per target (BasisK.gshift, uniform; G the smallest that holds C, at most a
//                                 wave), lane l of a group owns channel c0 + l; C > G takes further passes over the candidates.  A row run
//                                 is met G slots at a time: lane l tests slot base + l and, where it accepts, computes the weight, the
//                                 first plane and the 8 coefficients ONCE; the group then takes the accepted slots of the batch in
//                                 ascending order (a ballot), each handed to every lane by 9 shuffles, and a lane adds its channel of
//                                 that candidate's payload into 8 of its B accumulators.  So the whole group meets the candidates in
//                                 slot order, a rejected candidate costs one lane one test, and lanes without a channel (c >= C) still
//                                 test.  A lane's accumulators are a column of LDS, lds[b][thread]: consecutive lanes hit consecutive
//                                 banks and nobody reads or writes another lane's column, so there is no barrier.  The payload
//                                 xs[slot][c] is loaded coalesced across the group, out[row][b][c] stored likewise (non-temporal).
//   k_aggregate_basis_adjoint<Q>  a group of G lanes per particle in sorted-slot order, one register accumulator per lane and pass; the
//                                 rows that accept the particle are found the same way (adjoint_walk's tests, G rows at a time), and
//                                 h[row][b][c] is read in place through rowOf[] (ids[] for particle targets, the binning's perm[] for
//                                 query targets): h is not staged into row order.
// Groups are aligned inside a wave and a group's control flow is uniform, so a ballot's bits of the own group and a shuffle from a lane
// of the own group are defined whatever the other groups of the wave do.  Stores are lane-owned, by row; no atomics.  A candidate's 8
// planes are distinct (K >= 2), so the forward reads the 8 accumulators, then writes them.  The range guards (row < rows, j < n, c < C,
// b < B by the clamp of basis_axis) never fire; they stay so that no load or store can leave its array.
//
// Built on sph_aggregate.h without including it: the layering test lists the feature pairs that may include each other and this pair
// is not among them, so the translation unit includes sph_aggregate.h first (sph_engine.hip does) and the check below says so.
#pragma once
#include "sph_query.h"

#ifndef SPH_AGGREGATE_H
#error "sph_conv.h is built on sph_aggregate.h: include sph_aggregate.h before it"
#endif
#define SPH_CONV_H 1          // (sph_convgrad.h, which is built on this header, checks that it came first)

namespace sph {

constexpr int kBasisGrid = 0;                                   // SPH_BASIS_GRID
constexpr int kBasisMinSize = 2, kBasisMaxSize = 4;             // K; B = K^3 <= 64

struct BasisK {
    float R, half;           // the config's radius; 0.5f * (float)(K - 1)
    int weight, C, K;
    int gshift;              // log2 of the lanes per target
};

// The lanes per target: the smallest of 4, 8, 16, 32, 64 that holds C.
inline int basis_group_shift(int C) { return C <= 4 ? 2 : C <= 8 ? 3 : C <= 16 ? 4 : C <= 32 ? 5 : 6; }
// Threads per block: a lane's column is B floats of LDS.  K = 4 takes one wave per block (16 KiB; 10 blocks of a CU's 160 KiB), smaller
// grids four waves (K = 3: 27 KiB, K = 2: 8 KiB).
inline int basis_block(int K) { return K >= 4 ? 64 : kBlock; }

// One axis: the linear map of [-R, R] onto [0, K - 1], the cell and the two hat weights.  |d| < R for an accepted candidate, so the
// clamp is a guard.
__host__ __device__ inline void basis_axis(float d, float R, float half, int K, int& i, float& lo, float& hi) {
    const float u = d / R;
    const float g = (u + 1.0f) * half;
    int c = (g >= 0.0f) ? (int)fminf(g, (float)(K - 1)) : 0;   // (NaN and negatives go to 0 before the conversion)
    if (c > K - 2) c = K - 2;
    const float f = g - (float)c;
    i = c;
    lo = 1.0f - f;
    hi = f;
}

// The 8 corners of a candidate at offset d with weight w, in ascending plane: corner n has cx = n & 1, cy = (n >> 1) & 1, cz = n >> 2
// and the plane b0 + (cz K + cy) K + cx, b0 = (iz K + iy) K + ix the return value.
__host__ __device__ inline int basis_coefficients(float R, float half, int K, float w, float dx, float dy, float dz, float coef[8]) {
    int ix, iy, iz;
    float wx[2], wy[2], wz[2];
    basis_axis(dx, R, half, K, ix, wx[0], wx[1]);
    basis_axis(dy, R, half, K, iy, wy[0], wy[1]);
    basis_axis(dz, R, half, K, iz, wz[0], wz[1]);
#pragma unroll
    for (int n = 0; n < 8; ++n) coef[n] = w * ((wx[n & 1] * wy[(n >> 1) & 1]) * wz[n >> 2]);
    return (iz * K + iy) * K + ix;
}
__host__ __device__ inline int basis_plane(int b0, int K, int n) { return b0 + ((n >> 2) * K + ((n >> 1) & 1)) * K + (n & 1); }
__host__ __device__ inline void basis_corners(float R, float half, int K, float w, float dx, float dy, float dz, int b[8], float coef[8]) {
    const int b0 = basis_coefficients(R, half, K, w, dx, dy, dz, coef);
#pragma unroll
    for (int n = 0; n < 8; ++n) b[n] = basis_plane(b0, K, n);
}
__host__ __device__ inline float basis_add(float acc, float coef, float v) { return acc + coef * v; }

// The lanes of a group: lane `lane` of the group that starts at lane `base` of its wave; G = 1 << gshift lanes.
struct BasisGroup {
    uint32_t lane, base;
    int gshift;
};
__device__ __forceinline__ BasisGroup basis_group(int gshift) {
    const uint32_t inWave = threadIdx.x & 63u, lane = threadIdx.x & ((1u << gshift) - 1u);
    return BasisGroup{lane, inWave - lane, gshift};
}
// The own group's bits of a ballot: bit l is lane l of the group.
__device__ __forceinline__ unsigned long long basis_ballot(const BasisGroup& g, bool ok) {
    const unsigned long long all = __ballot(ok ? 1 : 0);
    return g.gshift >= 6 ? all : (all >> g.base) & ((1ull << (1u << g.gshift)) - 1ull);
}
// What lane `src` of the group computed for its candidate, in every lane of the group.
__device__ __forceinline__ void basis_take(const BasisGroup& g, uint32_t src, int b0, const float coef[8], int& b0Out, float out[8]) {
    const int from = (int)(g.base + src);
    b0Out = __shfl(b0, from);
#pragma unroll
    for (int n = 0; n < 8; ++n) out[n] = __shfl(coef[n], from);
}

// xs: the caller's values in slot order (k_aggregate_stage).  Dynamic LDS: B * blockDim.x floats; blockDim.x a multiple of 64.
template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_aggregate_basis(SimK k, NbK nb, BasisK bk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                            const int32_t* __restrict__ ids, const float4* __restrict__ own, const float4* __restrict__ points,
                                                            size_t rows, const float* __restrict__ xs, float* __restrict__ out, uint32_t* __restrict__ count) {
    extern __shared__ float lds[];
    const uint32_t tid = threadIdx.x, stride = blockDim.x;
    const BasisGroup grp = basis_group(bk.gshift);
    const size_t i = ((size_t)blockIdx.x * stride + tid) >> bk.gshift;
    float4 P;
    size_t row;
    bool walk;
    if (!query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk)) return;
    const bool self = (nb.flags & kAggSelf) != 0, fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    if (PARTICLES && fluidOnly && slot_ghost(own, (uint32_t)i)) walk = false;
    const uint32_t q = (uint32_t)i, G = 1u << bk.gshift;
    const int C = bk.C, K = bk.K, B = K * K * K;
    float* __restrict__ col = lds + tid;
    float* __restrict__ orow = out + row * (size_t)(B * C);
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    for (int c0 = 0; c0 < C; c0 += (int)G) {
        const int c = c0 + (int)grp.lane;
        const bool live = c < C;
        for (int b = 0; b < B; ++b) col[(uint32_t)b * stride] = 0.0f;
        uint32_t cnt = 0u;
        if (walk) {
            neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t base = qs; base < qe; base += G) {
                    const uint32_t j = base + grp.lane;
                    bool ok = false;
                    int b0 = 0;
                    float coef[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    if (j < qe) {
                        const float4 J = pv[2u * j];
                        float dx, dy, dz, r2;
                        ok = aggregate_accept(PARTICLES && j == q, self, P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2) && !(fluidOnly && slot_ghost(own, j));
                        if (ok) b0 = basis_coefficients(bk.R, bk.half, K, aggregate_weight(bk.weight, nb.R2, r2), dx, dy, dz, coef);
                    }
                    unsigned long long bits = basis_ballot(grp, ok);
                    cnt += (uint32_t)__popcll(bits);
                    while (bits) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(bits);
                        bits &= bits - 1ull;
                        int at;
                        float cf[8], a[8];
                        basis_take(grp, src, b0, coef, at, cf);
                        const uint32_t cand = base + src;
                        if (!live || cand >= nb.n || at < 0 || basis_plane(at, K, 7) >= B) continue;
                        const float v = xs[(size_t)cand * (size_t)C + (size_t)c];
#pragma unroll
                        for (int n = 0; n < 8; ++n) a[n] = col[(uint32_t)basis_plane(at, K, n) * stride];
#pragma unroll
                        for (int n = 0; n < 8; ++n) col[(uint32_t)basis_plane(at, K, n) * stride] = basis_add(a[n], cf[n], v);
                    }
                }
            });
        }
        if (live)
            for (int b = 0; b < B; ++b) __builtin_nontemporal_store(col[(uint32_t)b * stride], orow + (size_t)(b * C + c));
        if (c0 == 0 && grp.lane == 0u && count) count[row] = cnt;
    }
}

// h[row][B][C] in the caller's row numbering; rowOf[j] the row of sorted slot j of the row table (ids[] / perm[]); out[n][C] by particle
// id.  The tests are adjoint_walk's: the row is the TARGET and the particle the candidate, so d, r2 and w are the forward's bits.
template <bool QUERY>
__global__ __launch_bounds__(kBlock) void k_aggregate_basis_adjoint(SimK k, NbK nb, BasisK bk, const float4* __restrict__ pv, const int32_t* __restrict__ ids,
                                                                    const float4* __restrict__ own, AdjRows rows, const uint32_t* __restrict__ rowOf,
                                                                    const float* __restrict__ h, float* __restrict__ out) {
    constexpr uint32_t STRIDE = QUERY ? 1u : 2u;
    const BasisGroup grp = basis_group(bk.gshift);
    const size_t t = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> bk.gshift;
    if (t >= (size_t)nb.n) return;
    const uint32_t q = (uint32_t)t, G = 1u << bk.gshift;
    float4 P;
    uint32_t id;
    if (!adjoint_particle(nb, pv, ids, q, P, id)) return;
    const bool self = !QUERY && (nb.flags & kAggSelf) != 0, fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    const bool walk = !(fluidOnly && slot_ghost(own, q));                   // a ghost under FLUID_ONLY is nobody's candidate
    const int C = bk.C, K = bk.K, B = K * K * K;
    float* __restrict__ orow = out + (size_t)id * (size_t)C;
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    for (int c0 = 0; c0 < C; c0 += (int)G) {
        const int c = c0 + (int)grp.lane;
        const bool live = c < C;
        float acc = 0.0f;
        if (walk) {
            neighbor_rows(k, rows.start, nb.s, rows.end, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t base = qs; base < qe; base += G) {
                    const uint32_t j = base + grp.lane;
                    bool ok = false;
                    int b0 = 0;
                    uint32_t r = 0u;
                    float coef[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    if (j < qe) {
                        const float4 X = rows.pos[STRIDE * j];
                        float dx, dy, dz, r2;
                        ok = aggregate_accept(!QUERY && j == q, self, X.x, X.y, X.z, P.x, P.y, P.z, nb.R2, dx, dy, dz, r2) &&
                             !(!QUERY && fluidOnly && slot_ghost(own, j));      // (a ghost target's row is empty)
                        if (ok) {
                            r = rowOf[j];
                            b0 = basis_coefficients(bk.R, bk.half, K, aggregate_weight(bk.weight, nb.R2, r2), dx, dy, dz, coef);
                        }
                    }
                    unsigned long long bits = basis_ballot(grp, ok);
                    while (bits) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(bits);
                        bits &= bits - 1ull;
                        int at;
                        float cf[8];
                        basis_take(grp, src, b0, coef, at, cf);
                        const uint32_t from = (uint32_t)__shfl((int)r, (int)(grp.base + src));
                        if (!live || from >= rows.end || at < 0 || basis_plane(at, K, 7) >= B) continue;
                        const float* __restrict__ hrow = h + (size_t)from * (size_t)(B * C) + (size_t)c;
#pragma unroll
                        for (int n = 0; n < 8; ++n) acc = basis_add(acc, cf[n], hrow[(size_t)(basis_plane(at, K, n) * C)]);
                    }
                }
            });
        }
        if (live) orow[c] = acc;
    }
}

}  // namespace sph
