// sph_convgrad.h -- position gradients of the filter-grid basis sums: with L = sum g . A, A the basis sums of sph_conv.h as a function of
// the positions, the pair term e(i -> j) = dL/dd for target i and accepted candidate j (d = x_j - x_i), summed into dL/dx of the particles
// and of the query points (no reference counterpart).  Feature layer above sph_aggregate.h, sph_conv.h and
// sph_posgrad.h: grid, radius rules, stencil, candidate order, acceptance (aggregate_accept), FLUID_ONLY, the weight (aggregate_weight),
// the staged payload (k_aggregate_stage), the point binning and the row tables of the transposed walk (AdjRows) are the first header's;
// the filter grid (basis_axis, basis_plane, BasisK, the group's ballot) the second's; the weight's derivative (posgrad_w1), the group
// size (posgrad_group_shift), the butterfly (posgrad_reduce, posgrad_reduce_host) and the three modes the third's.  Every product and sum
// is rounded on its own (no fmaf: the build's -ffp-contract=off).
//
//   convgrad_slope / _corner / _step / _e   __host__ __device__ per-term functions: sph_aggregate_basis_posgrad_host runs them too
//   convgrad_pair_host                      the twin of a group's partial sums, their butterfly and the assembly
//   k_aggregate_basis_posgrad<MODE, T>      a group of G = 4 .. 64 lanes per target (BasisK.gshift, uniform; G the smallest that holds C,
//                                           at most a wave), lane l of a group owns the channels l, l + G (T = 1 or 2: C <= 128).  A row
//                                           run is met G slots at a time: lane l tests slot base + l and, where it accepts, runs
//                                           basis_axis ONCE per axis (on d, and for particle targets on -d); the group then takes the
//                                           accepted slots of the batch in ascending order (a ballot), the geometry handed to every lane
//                                           by shuffles.  A candidate touches 8 planes of g: every lane folds its channels of them into
//                                           four partial sums (the hat sum and its three slopes), a xor-butterfly leaves the same bits of
//                                           the four sums in every lane, and every lane assembles the pair term and adds it into its own
//                                           copy of the three accumulators.  Lane 0 stores the row.
//                                           MODE kPosParticles: particle targets in sorted-slot order, both directions of every pair in
//                                           one walk; kPosPoints: the query points' own gradient; kPosCandidates: a group per particle
//                                           over the binned query points.
// g is read IN PLACE, 8 planes per candidate: the target's own row through its row number, a candidate's row through rowOf[] (ids[] for
// particle targets, the binning's perm[] for query targets) as the basis adjoint reads h; a lane reads g[row][b][c] for its own c, so the
// group's loads of one plane are contiguous.  The target's own values stay in registers; a candidate's values xs[slot][c] are loaded
// coalesced across the group.  No LDS.  Groups are aligned inside a wave and a group's control flow is uniform, so a ballot's bits of the
// own group and a shuffle from a lane of the own group are defined whatever the other groups of the wave do.  Stores are lane-owned, by
// row; no atomics.  The range guards (row < rows, candidate < n, c < C, b < B by the clamp of basis_axis) never fire; they stay so that
// no load or store can leave its array.
//
// Built on sph_aggregate.h, sph_conv.h and sph_posgrad.h without including them (as those two are on the first): the translation unit
// includes them first, in that order.
#pragma once
#include "sph_query.h"

#if !defined(SPH_AGGREGATE_H) || !defined(SPH_CONV_H) || !defined(SPH_POSGRAD_H)
#error "sph_convgrad.h is built on sph_aggregate.h, sph_conv.h and sph_posgrad.h: include them before it, in that order"
#endif

namespace sph {

// The slope of a hat along its axis: g = (d / R + 1) * half, so dg/dd = half / R (one division); lo falls with -s, hi rises with +s.
__host__ __device__ inline float convgrad_slope(float R, float half) { return half / R; }

// Corner n (cx = n & 1, cy = (n >> 1) & 1, cz = n >> 2) of a candidate whose axes gave the hat weights wx, wy, wz ([0] lo, [1] hi):
// c[0] the hat product WITHOUT the weight, c[1 .. 3] its derivative along x, y, z (the slope in place of that axis' hat weight).
__host__ __device__ inline void convgrad_corner(int n, float s, const float wx[2], const float wy[2], const float wz[2], float c[4]) {
    const int cx = n & 1, cy = (n >> 1) & 1, cz = n >> 2;
    const float sx = cx ? s : -s, sy = cy ? s : -s, sz = cz ? s : -s;
    c[0] = (wx[cx] * wy[cy]) * wz[cz];
    c[1] = (sx * wy[cy]) * wz[cz];
    c[2] = (wx[cx] * sy) * wz[cz];
    c[3] = (wx[cx] * wy[cy]) * sz;
}
// One corner of one channel into a lane's four partial sums: u = g * x.
__host__ __device__ inline void convgrad_step(float p[4], const float c[4], float gv, float xv) {
    const float u = gv * xv;
    p[0] = p[0] + c[0] * u;
    p[1] = p[1] + c[1] * u;
    p[2] = p[2] + c[2] * u;
    p[3] = p[3] + c[3] * u;
}
// The pair term from the reduced sums s = (q, p_x, p_y, p_z): f = w1 * q, e_a = (f * d_a) + w * p_a.
__host__ __device__ inline void convgrad_e(int weight, float R2, float r2, float dx, float dy, float dz, const float s[4], float e[3]) {
    const float w = aggregate_weight(weight, R2, r2), f = posgrad_w1(weight, R2, r2) * s[0];
    e[0] = (f * dx) + w * s[1];
    e[1] = (f * dy) + w * s[2];
    e[2] = (f * dz) + w * s[3];
}

// One direction of one pair on the host, in the kernel's order: grow the g row of the pair's target ([B][C]), x the candidate's values.
// Lane l of G sums its channels c = l, l + G, .. ascending and inside a channel the corners n = 0 .. 7 ascending, from +0; then the
// butterfly of each of the four sums.
inline void convgrad_pair_host(const BasisK& bk, float R2, float dx, float dy, float dz, float r2, const float* grow, const float* x, float e[3]) {
    const int C = bk.C, K = bk.K, G = 1 << posgrad_group_shift(C);
    int ix, iy, iz;
    float wx[2], wy[2], wz[2], cf[8][4], part[4][kPosMaxGroup], s[4];
    basis_axis(dx, bk.R, bk.half, K, ix, wx[0], wx[1]);
    basis_axis(dy, bk.R, bk.half, K, iy, wy[0], wy[1]);
    basis_axis(dz, bk.R, bk.half, K, iz, wz[0], wz[1]);
    const int b0 = (iz * K + iy) * K + ix;
    const float slope = convgrad_slope(bk.R, bk.half);
    for (int n = 0; n < 8; ++n) convgrad_corner(n, slope, wx, wy, wz, cf[n]);
    for (int l = 0; l < G; ++l) {
        float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = l; c < C; c += G)
            for (int n = 0; n < 8; ++n) convgrad_step(p, cf[n], grow[(size_t)basis_plane(b0, K, n) * (size_t)C + (size_t)c], x[c]);
        for (int a = 0; a < 4; ++a) part[a][l] = p[a];
    }
    for (int a = 0; a < 4; ++a) s[a] = posgrad_reduce_host(part[a], G);
    convgrad_e(bk.weight, R2, r2, dx, dy, dz, s, e);
}

// What a tester lane found out about its candidate along one direction: the first plane and the three upper hat weights (lo = 1 - hi,
// the subtraction basis_axis itself makes).
struct ConvGeo {
    int b0;
    float hx, hy, hz;
};
__device__ __forceinline__ ConvGeo convgrad_geo(const BasisK& bk, float dx, float dy, float dz) {
    int ix, iy, iz;
    float lo, hx, hy, hz;
    basis_axis(dx, bk.R, bk.half, bk.K, ix, lo, hx);
    basis_axis(dy, bk.R, bk.half, bk.K, iy, lo, hy);
    basis_axis(dz, bk.R, bk.half, bk.K, iz, lo, hz);
    return ConvGeo{(iz * bk.K + iy) * bk.K + ix, hx, hy, hz};
}
__device__ __forceinline__ ConvGeo convgrad_take(const ConvGeo& g, int from) {
    return ConvGeo{__shfl(g.b0, from), __shfl(g.hx, from), __shfl(g.hy, from), __shfl(g.hz, from)};
}
// A lane's share of one direction: its T channels of the 8 planes of grow (the row's g, at the lane's first channel) against xv[t],
// reduced over the group.  ok false (a guard fired): the sums stay +0, the butterfly still runs (uniform control flow).
template <int T>
__device__ __forceinline__ void convgrad_sums(const BasisK& bk, const ConvGeo& geo, float slope, bool ok, const float* __restrict__ grow, int lane, const float xv[T],
                                              float s[4]) {
    const int C = bk.C, K = bk.K, G = 1 << bk.gshift;
    const float wx[2] = {1.0f - geo.hx, geo.hx}, wy[2] = {1.0f - geo.hy, geo.hy}, wz[2] = {1.0f - geo.hz, geo.hz};
    s[0] = s[1] = s[2] = s[3] = 0.0f;
    if (ok) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int c = lane + t * G;
            if (c >= C) continue;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                float cf[4];
                convgrad_corner(n, slope, wx, wy, wz, cf);
                convgrad_step(s, cf, grow[(size_t)(basis_plane(geo.b0, K, n) * C + t * G)], xv[t]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] = posgrad_reduce(s[a], bk.gshift);
}

// rows: the targets (n sorted slots, m points, n sorted slots); adj: the binned points (kPosCandidates only).  vs: the values in slot
// order (kPosCandidates: the caller's values by id); g: the caller's g[rows][B][C], never staged; rowOf[j]: the g row of candidate slot j
// (ids[] for kPosParticles, perm[] for kPosCandidates, unused for kPosPoints).  out float32[rows][3] by particle id or by point.
template <int MODE, int T>
__global__ __launch_bounds__(kBlock) void k_aggregate_basis_posgrad(SimK k, NbK nb, BasisK bk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                                    const int32_t* __restrict__ ids, const float4* __restrict__ own, const float4* __restrict__ points,
                                                                    size_t rows, AdjRows adj, const uint32_t* __restrict__ rowOf, const float* __restrict__ vs,
                                                                    const float* __restrict__ g, float* __restrict__ out) {
    constexpr bool OWN_G = MODE != kPosCandidates, OWN_V = MODE != kPosPoints, CAND_G = MODE != kPosPoints, CAND_V = MODE != kPosCandidates;
    const int gshift = bk.gshift, C = bk.C, K = bk.K, B = K * K * K;
    const uint32_t G = 1u << gshift, lane = threadIdx.x & (G - 1u), base0 = (threadIdx.x & 63u) - lane;
    const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> gshift;
    const bool fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    const size_t BC = (size_t)(B * C);
    float4 P;
    size_t row, ownV = 0;
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
        ownV = i * (size_t)C;
    }
    const uint32_t q = (uint32_t)i;
    const float* __restrict__ gOwn = OWN_G ? g + row * BC + (size_t)lane : g;       // the target's own row of g, at the lane's first channel
    float mv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c = (int)lane + t * (int)G;
        mv[t] = (OWN_V && c < C) ? vs[ownV + (size_t)c] : 0.0f;
    }
    const float slope = convgrad_slope(bk.R, bk.half);
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (walk) {
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        const uint32_t end = MODE == kPosCandidates ? adj.end : nb.n;
        neighbor_rows(k, MODE == kPosCandidates ? adj.start : cellStart, nb.s, end, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t base = qs; base < qe; base += G) {
                const uint32_t j = base + lane;
                bool ok = false;
                float dx = 0.0f, dy = 0.0f, dz = 0.0f, r2 = 0.0f;
                uint32_t r = 0u;
                ConvGeo out0{0, 0.0f, 0.0f, 0.0f}, in0{0, 0.0f, 0.0f, 0.0f};
                if (j < qe) {
                    if (MODE == kPosCandidates) {                               // the point is the TARGET: d = x_k - x_i, the forward's bits
                        const float4 X = adj.pos[j];
                        ok = aggregate_accept(false, false, X.x, X.y, X.z, P.x, P.y, P.z, nb.R2, dx, dy, dz, r2);
                    } else {
                        const float4 J = pv[2u * j];
                        ok = !(MODE == kPosParticles && j == q) && aggregate_accept(false, false, P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2) &&
                             !(fluidOnly && slot_ghost(own, j));
                    }
                    if (ok) {
                        out0 = convgrad_geo(bk, dx, dy, dz);
                        if (MODE == kPosParticles) in0 = convgrad_geo(bk, -dx, -dy, -dz);     // (not mirrored: (-u + 1) * half rounds on its own)
                        if (CAND_G) r = rowOf[j];
                    }
                }
                unsigned long long bits = posgrad_ballot(base0, gshift, ok);
                while (bits) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(bits);
                    bits &= bits - 1ull;
                    const int from = (int)(base0 + src);
                    const float ex = __shfl(dx, from), ey = __shfl(dy, from), ez = __shfl(dz, from), e2 = __shfl(r2, from);
                    const ConvGeo geo = convgrad_take(out0, from);
                    const uint32_t cand = base + src, crow = CAND_G ? (uint32_t)__shfl((int)r, from) : 0u;
                    const bool inRange = cand < end && geo.b0 >= 0 && basis_plane(geo.b0, K, 7) < B && (!CAND_G || (size_t)crow < (MODE == kPosParticles ? rows : (size_t)adj.end));
                    float xv[T], s[4], e[3];
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int c = (int)lane + t * (int)G;
                        xv[t] = (CAND_V && inRange && c < C) ? vs[(size_t)cand * (size_t)C + (size_t)c] : mv[t];
                    }
                    // e(target -> candidate): the g row of the target.  kPosCandidates: the target is the point, its row the candidate's.
                    convgrad_sums<T>(bk, geo, slope, inRange, OWN_G ? gOwn : g + (size_t)crow * BC + (size_t)lane, (int)lane, xv, s);
                    convgrad_e(bk.weight, nb.R2, e2, ex, ey, ez, s, e);
                    if (MODE == kPosParticles) {                                // e(j -> k): g[j], x[k], -d (exact), the same r2 and w
                        const ConvGeo back = convgrad_take(in0, from);
                        const bool inBack = inRange && back.b0 >= 0 && basis_plane(back.b0, K, 7) < B;
                        float b[3];
                        convgrad_sums<T>(bk, back, slope, inBack, g + (size_t)crow * BC + (size_t)lane, (int)lane, mv, s);
                        convgrad_e(bk.weight, nb.R2, e2, -ex, -ey, -ez, s, b);
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
