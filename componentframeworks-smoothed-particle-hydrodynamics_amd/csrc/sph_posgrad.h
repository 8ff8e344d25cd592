// sph_posgrad.h -- position gradients of the neighbourhood sums: with L = sum g . out, out the SUM of sph_aggregate.h as a function of the
// positions, the pair term e(i -> j) = dL/dd for target i and accepted candidate j (d = x_j - x_i), summed into dL/dx of the particles
// and of the query points (no reference counterpart).  Feature layer above sph_aggregate.h: grid, radius rules,
// stencil, candidate order, acceptance (neighbor_offset through aggregate_accept), FLUID_ONLY, the weight (aggregate_weight), the
// reduced value (aggregate_value), the staged payload (k_aggregate_stage, k_adjoint_stage), the point binning (k_adjoint_bin / _scatter /
// _rank) and the row tables of the transposed walk (AdjRows) are that header's.  Every product and sum is rounded on its own (no fmaf:
// the build's -ffp-contract=off).
//
//   posgrad_w1 / _dot / _q / _e      __host__ __device__ per-term functions: sph_aggregate_posgrad_host runs them too
//   posgrad_reduce_host              the twin of the group's xor-butterfly
//   k_aggregate_posgrad<MODE, M, T>  a group of G = 4 .. 64 lanes per target (PosK.gshift, uniform; G the smallest that holds C, at most
//                                    a wave), lane l of a group owns the channels l, l + G (T = 1 or 2 channels per lane: C <= 128).  A row
//                                    run is met G slots at a time: lane l tests slot base + l; the group then takes the accepted slots of
//                                    the batch in ascending order (a ballot), d and r2 handed to every lane by 4 shuffles; every lane
//                                    forms its partial dots over its own channels, a xor-butterfly (offsets 1, 2, .. G / 2) leaves the
//                                    same bits of every dot in every lane, and every lane assembles the pair term and adds it into its
//                                    own copy of the three accumulators.  Lane 0 stores the row.
//                                    MODE kPosParticles: particle targets in sorted-slot order, both directions of every pair in one walk
//                                    (vs: values, gs: g, both in slot order); kPosPoints: the query points' own gradient (vs: values in
//                                    slot order, gs: the caller's g by point); kPosCandidates: a group per particle over the binned
//                                    query points (vs: the caller's values by id, gs: g in binned order).  M: g has the moment planes.
// The target's own rows (g and, where needed, values) stay in registers; a candidate's payload is loaded coalesced across the group.
// Groups are aligned inside a wave and a group's control flow is uniform, so a ballot's bits of the own group and a shuffle from a lane
// of the own group are defined whatever the other groups of the wave do.  Stores are lane-owned, by row; no atomics.  The range guards
// (row < rows, candidate < n, c < C) never fire; they stay so that no load or store can leave its array.
//
// Built on sph_aggregate.h without including it (as sph_conv.h): the translation unit includes sph_aggregate.h first.
#pragma once
#include "sph_query.h"

#ifndef SPH_AGGREGATE_H
#error "sph_posgrad.h is built on sph_aggregate.h: include sph_aggregate.h before it"
#endif
#define SPH_POSGRAD_H 1       // (sph_convgrad.h, which is built on this header, checks that it came first)

namespace sph {

constexpr int kPosParticles = 0, kPosPoints = 1, kPosCandidates = 2;
constexpr int kPosMaxGroup = 64;

struct PosK {
    int weight, C, delta;
    int gshift;              // log2 of the lanes per target
};

// The lanes per target: the smallest of 4, 8, 16, 32, 64 that holds C; a function of C alone, so that the order of the channel dot is.
__host__ __device__ inline int posgrad_group_shift(int C) { return C <= 4 ? 2 : C <= 8 ? 3 : C <= 16 ? 4 : C <= 32 ? 5 : 6; }

// Twice the derivative of the weight with respect to r2 (the 2 of d r2 / d d = 2 d folded in): ONE 0, POLY6 -6 (R2 - r2)^2.
__host__ __device__ inline float posgrad_w1(int weight, float R2, float r2) {
    if (weight == kAggWeightOne) return 0.0f;
    const float t = R2 - r2;
    return -6.0f * (t * t);
}
// One step of a lane's partial channel dot.
__host__ __device__ inline float posgrad_dot(float part, float g, float v) { return part + g * v; }
// q = s0 (+ d . s with MOMENTS), left to right.
__host__ __device__ inline float posgrad_q(bool moments, const float s[4], float dx, float dy, float dz) {
    if (!moments) return s[0];
    return ((s[0] + dx * s[1]) + dy * s[2]) + dz * s[3];
}
// One component of e: f = w1 * q.
__host__ __device__ inline float posgrad_e(bool moments, float f, float d, float w, float sa) {
    const float e = f * d;
    return moments ? e + w * sa : e;
}
// The pair term of a target whose dots are s[0 .. planes) towards a candidate at offset d.
__host__ __device__ inline void posgrad_pair(bool moments, int weight, float R2, float r2, float dx, float dy, float dz, const float s[4], float e[3]) {
    const float w = aggregate_weight(weight, R2, r2), f = posgrad_w1(weight, R2, r2) * posgrad_q(moments, s, dx, dy, dz);
    e[0] = posgrad_e(moments, f, dx, w, moments ? s[1] : 0.0f);
    e[1] = posgrad_e(moments, f, dy, w, moments ? s[2] : 0.0f);
    e[2] = posgrad_e(moments, f, dz, w, moments ? s[3] : 0.0f);
}

// The group's butterfly on the host: part[0 .. G) the lanes' partial sums; every lane ends with the same bits, part[0] is returned.
inline float posgrad_reduce_host(float* part, int G) {
    float next[kPosMaxGroup];
    for (int off = 1; off < G; off <<= 1) {
        for (int l = 0; l < G; ++l) next[l] = part[l] + part[l ^ off];
        for (int l = 0; l < G; ++l) part[l] = next[l];
    }
    return part[0];
}
// s[p] = the dot over the channels of g[p][c] * value(delta, a[c], b[c]) in the kernel's order: lane l sums c = l, l + G, .. ascending
// from +0, then the butterfly.
inline void posgrad_dots_host(int C, int planes, bool delta, const float* g, const float* a, const float* b, float s[4]) {
    const int G = 1 << posgrad_group_shift(C);
    float part[kPosMaxGroup];
    for (int p = 0; p < planes; ++p) {
        for (int l = 0; l < G; ++l) {
            part[l] = 0.0f;
            for (int c = l; c < C; c += G) part[l] = posgrad_dot(part[l], g[p * C + c], aggregate_value(delta, a[c], delta ? b[c] : 0.0f));
        }
        s[p] = posgrad_reduce_host(part, G);
    }
    for (int p = planes; p < 4; ++p) s[p] = 0.0f;
}

__device__ __forceinline__ float posgrad_reduce(float v, int gshift) {
    for (int off = 1; off < (1 << gshift); off <<= 1) v = v + __shfl_xor(v, off);
    return v;
}
// The own group's bits of a ballot: bit l is lane l of the group that starts at lane `base` of its wave.
__device__ __forceinline__ unsigned long long posgrad_ballot(uint32_t base, int gshift, bool ok) {
    const unsigned long long all = __ballot(ok ? 1 : 0);
    return gshift >= 6 ? all : (all >> base) & ((1ull << (1u << gshift)) - 1ull);
}

// rows: the targets (n sorted slots, m points, n sorted slots); adj: the binned points (kPosCandidates only).  out float32[rows][3] by
// particle id or by point.
template <int MODE, bool MOMENTS, int T>
__global__ __launch_bounds__(kBlock) void k_aggregate_posgrad(SimK k, NbK nb, PosK pk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                              const int32_t* __restrict__ ids, const float4* __restrict__ own, const float4* __restrict__ points,
                                                              size_t rows, AdjRows adj, const float* __restrict__ vs, const float* __restrict__ gs,
                                                              float* __restrict__ out) {
    constexpr int PLANES = MOMENTS ? 4 : 1;
    constexpr bool NEED_G = MODE != kPosCandidates, NEED_V = MODE != kPosPoints;     // which of the target's own rows stay in registers
    const int gshift = pk.gshift, C = pk.C;
    const uint32_t G = 1u << gshift, lane = threadIdx.x & (G - 1u), base0 = (threadIdx.x & 63u) - lane;
    const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> gshift;
    const bool fluidOnly = (nb.flags & kAggFluidOnly) != 0, delta = MODE == kPosParticles && pk.delta != 0;
    const size_t PC = (size_t)(PLANES * C);
    float4 P;
    size_t row, ownG = 0, ownV = 0;
    bool walk;
    if (MODE == kPosCandidates) {
        uint32_t id;
        if (i >= rows || !adjoint_particle(nb, pv, ids, (uint32_t)i, P, id)) return;
        row = id;
        walk = !(fluidOnly && slot_ghost(own, (uint32_t)i));                   // a ghost under FLUID_ONLY is nobody's candidate
        ownV = (size_t)id * (size_t)C;
    } else {
        if (!query_target<MODE == kPosParticles>(pv, ids, points, rows, i, P, row, walk)) return;
        if (MODE == kPosParticles && fluidOnly && slot_ghost(own, (uint32_t)i)) walk = false;
        ownG = (MODE == kPosParticles ? i : row) * PC;
        ownV = i * (size_t)C;
    }
    const uint32_t q = (uint32_t)i;
    float mg[PLANES][T], mv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c = (int)lane + t * (int)G;
        mv[t] = (NEED_V && c < C) ? vs[ownV + (size_t)c] : 0.0f;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) mg[p][t] = (NEED_G && c < C) ? gs[ownG + (size_t)(p * C + c)] : 0.0f;
    }
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (walk) {
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        const uint32_t end = MODE == kPosCandidates ? adj.end : nb.n;
        neighbor_rows(k, MODE == kPosCandidates ? adj.start : cellStart, nb.s, end, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t base = qs; base < qe; base += G) {
                const uint32_t j = base + lane;
                bool ok = false;
                float dx = 0.0f, dy = 0.0f, dz = 0.0f, r2 = 0.0f;
                if (j < qe) {
                    if (MODE == kPosCandidates) {                               // the point is the TARGET: d = x_k - x_i, the forward's bits
                        const float4 X = adj.pos[j];
                        ok = aggregate_accept(false, false, X.x, X.y, X.z, P.x, P.y, P.z, nb.R2, dx, dy, dz, r2);
                    } else {
                        const float4 J = pv[2u * j];
                        ok = !(MODE == kPosParticles && j == q) && aggregate_accept(false, false, P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2) &&
                             !(fluidOnly && slot_ghost(own, j));
                    }
                }
                unsigned long long bits = posgrad_ballot(base0, gshift, ok);
                while (bits) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(bits);
                    bits &= bits - 1ull;
                    const int from = (int)(base0 + src);
                    const float ex = __shfl(dx, from), ey = __shfl(dy, from), ez = __shfl(dz, from), e2 = __shfl(r2, from);
                    const uint32_t cand = base + src;
                    float sOut[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sIn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (cand < end) {
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const int c = (int)lane + t * (int)G;
                            if (c >= C) continue;
                            if (MODE == kPosCandidates) {
                                const float* __restrict__ grow = gs + (size_t)cand * PC + (size_t)c;
#pragma unroll
                                for (int p = 0; p < PLANES; ++p) sOut[p] = posgrad_dot(sOut[p], grow[p * C], mv[t]);
                            } else {
                                const float vj = vs[(size_t)cand * (size_t)C + (size_t)c];
                                const float vOut = aggregate_value(delta, vj, mv[t]);
#pragma unroll
                                for (int p = 0; p < PLANES; ++p) sOut[p] = posgrad_dot(sOut[p], mg[p][t], vOut);
                                if (MODE == kPosParticles) {
                                    const float* __restrict__ grow = gs + (size_t)cand * PC + (size_t)c;
                                    const float vIn = aggregate_value(delta, mv[t], vj);
#pragma unroll
                                    for (int p = 0; p < PLANES; ++p) sIn[p] = posgrad_dot(sIn[p], grow[p * C], vIn);
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) {
                        sOut[p] = posgrad_reduce(sOut[p], gshift);
                        if (MODE == kPosParticles) sIn[p] = posgrad_reduce(sIn[p], gshift);
                    }
                    float e[3];
                    posgrad_pair(MOMENTS, pk.weight, nb.R2, e2, ex, ey, ez, sOut, e);
                    if (MODE == kPosParticles) {                                // e(j -> k) with d' = -d (exact), minus e(k -> j)
                        float b[3];
                        posgrad_pair(MOMENTS, pk.weight, nb.R2, e2, -ex, -ey, -ez, sIn, b);
                        ax = ax + (b[0] - e[0]); ay = ay + (b[1] - e[1]); az = az + (b[2] - e[2]);
                    } else if (MODE == kPosPoints) {
                        ax = ax - e[0]; ay = ay - e[1]; az = az - e[2];
                    } else {
                        ax = ax + e[0]; ay = ay + e[1]; az = az + e[2];
                    }
                }
            }
        });
    }
    if (lane == 0u) {
        float* __restrict__ orow = out + row * 3u;
        orow[0] = ax; orow[1] = ay; orow[2] = az;
    }
}

}  // namespace sph
