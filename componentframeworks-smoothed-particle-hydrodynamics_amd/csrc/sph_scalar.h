// sph_scalar.h -- diffusing scalar fields carried by the particles: dye, heat (no reference counterpart).
//
// K <= kScalarMax fp32 channels per particle, stored particle-major (c[i * K + k]) in the caller's order: a value moves with its
// particle for free and exchanges with the particle's neighbours through the Brookshaw / Cleary-Monaghan Laplacian with the spiky
// gradient.  One substep, on the sorted copy of the substep's ENTRY state (the grid dispatch_one has just built for the SPH pass):
//
//   k_scalar_gather   sC[q] = (c[id(q)][0..K), g) in slot order, g = 0 for a ghost record (isGhost != 0), 1 otherwise; thread 0 also
//                     clears the diffusion number of the substep before
//   k_scalar_sweep    one target per lane in slot order: the candidates of a probe at x_i (sample_rows: the clamped cell of x_i,
//                     9 rows in (dz, dy) order, slots ascending, slot i itself skipped), scalar_pair per candidate, scalar_finish,
//                     c[id(q)] written in place.  It reads the sorted copies only (pv, sC), so no second value buffer is needed.
//
// scalar_pair / scalar_finish / scalar_make_coef are __host__ __device__: sph_scalars_step_host runs the same functions in plain
// loops.  fp32, every operation rounded on its own except the explicit fmaf()s (-ffp-contract=off); division and sqrtf are IEEE.
// No float atomics: the only atomic is the maximum of the diffusion number, taken on the bits of a non-negative float.
//
//   k_scalar_sweep_staged   the same with the block's candidate rows staged in LDS (SPH_OPT_SCALAR_SWEEP 1)
//   k_scalar_sample_*       Shepard value of a channel at probe points / on a lattice (one point per thread)
//   k_scalar_stat_view      a channel laid out as the statistics kernels' input (sph_scalars_moments)
//   k_scalar_seed     channel 0 = padB of the records (the reference's marble dye), the other channels 0
//   k_scalar_paint    one thread per particle of the engine's own state arrays (or of the 80-byte array while that is the valid
//                     state): SET or ADD inside a sphere
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "sph_query.h"    // HostGrid of the *_host twin
#include "sph_sample.h"   // sample_rows

namespace sph {

constexpr int kScalarMax = 4;          // SPH_MAX_SCALAR_CHANNELS
constexpr int kScalarSet = 0, kScalarAdd = 1;   // SPH_SCALAR_SET / SPH_SCALAR_ADD

// What the kernels read of the coefficients, in DEVICE memory: a replayed graph sees a later sph_scalars_set_coefficients.  (kLap
// depends on param_mass and param_h, which are part of a graph's key: it is a launch argument.)
struct ScalarCoef {
    float d[kScalarMax];
    float lambda[kScalarMax];
    float dmax;                        // max_k D_k
    float pad[3];
};
static_assert(sizeof(ScalarCoef) == 48, "ScalarCoef is 48 bytes");

// kLap = (float)(2 m 45 / (pi h^6)) = (float)((90 m) / (pi ((h^2 h^2) h^2))), in double on the host.
inline float scalar_klap(float mass, float h) {
    const double hd = (double)h, h2 = hd * hd;
    return (float)((90.0 * (double)mass) / (3.14159265358979323846 * ((h2 * h2) * h2)));
}
// coeffs = D_0 .. D_{K-1}, lambda_0 .. lambda_{K-1}
inline void scalar_make_coef(int K, const float* coeffs, ScalarCoef& c) {
    c.dmax = 0.0f;
    for (int k = 0; k < kScalarMax; ++k) {
        c.d[k] = k < K ? coeffs[k] : 0.0f;
        c.lambda[k] = k < K ? coeffs[K + k] : 0.0f;
        if (c.d[k] > c.dmax) c.dmax = c.d[k];
    }
    c.pad[0] = c.pad[1] = c.pad[2] = 0.0f;
}

// One candidate j of target i.  wj = 1/rho_j, or 0 for a ghost record: only pairs with 0 < r2 < h2 and wj > 0 take part.
// w is bitwise symmetric in i and j (the squares of x_i - x_j and of x_j - x_i are the same floats, products commute).
template <int K>
__host__ __device__ inline void scalar_pair(float h, float h2, float xi, float yi, float zi, float wi, const float* ci,
                                            float xj, float yj, float zj, float wj, const float* cj, float (&a)[K], float& W) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const float r2 = dot3(dx, dy, dz, dx, dy, dz);
    if (!(r2 > 0.0f && r2 < h2 && wj > 0.0f)) return;
    const float r = sqrtf(r2);
    const float u = h - r;
    const float G = ((u * u) * r) / (r2 + 0.01f * h2);
    const float w = (wi * wj) * G;
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = fmaf(w, cj[k] - ci[k], a[k]);
    W += w;
}

// c_ik' = c_ik + dt * ((D_k * kLap) * a_k - lambda_k * c_ik) and the diffusion number s_i = (dt * (Dmax * kLap)) * W: multiplies and adds, no fma.
template <int K>
__host__ __device__ inline float scalar_finish(const ScalarCoef& co, float kLap, float dt, const float* ci, const float (&a)[K], float W, float* out) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = ci[k] + dt * (((co.d[k] * kLap) * a[k]) - (co.lambda[k] * ci[k]));
    return (dt * (co.dmax * kLap)) * W;
}

// state[0]: bits of the largest diffusion number of the last substep's targets (cleared by the substep's gather; state == nullptr:
// the gather of the sampling entry points, which leaves the number alone)
template <int K>
__global__ __launch_bounds__(kBlock) void k_scalar_gather(const float4* __restrict__ own, const float* __restrict__ c, float* __restrict__ sC,
                                                          uint32_t* __restrict__ state, uint32_t idBase, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q == 0u && state) state[0] = 0u;
    if (q >= n) return;
    const float4 o = own[q];
    const uint32_t id = fbits(o.w) - idBase;
    const bool ok = id < n;                                            // (always: ids are idBase + [0, n))
    float* d = sC + (size_t)q * (K + 1);
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = ok ? c[(size_t)id * K + k] : 0.0f;
    d[K] = (ok && !(fbits(o.z) & F_GHOSTNZ)) ? 1.0f : 0.0f;
}

// Candidate slot j of target slot q from global memory.
template <int K>
__device__ __forceinline__ void scalar_candidate_global(const SimK& k, const float4* __restrict__ pv, const float* __restrict__ sC, const float4& P,
                                                        const float (&ci)[K], uint32_t j, float (&a)[K], float& W) {
    const float4 J = pv[2u * j];
    const float* cj = sC + (size_t)j * (K + 1);
    float cjv[K];
#pragma unroll
    for (int u = 0; u < K; ++u) cjv[u] = cj[u];
    scalar_pair<K>(k.h, k.h2, P.x, P.y, P.z, P.w, ci, J.x, J.y, J.z, cj[K] > 0.0f ? J.w : 0.0f, cjv, a, W);
}

// Is slot q a target?  Loads its position record and its gathered values.
template <int K>
__device__ __forceinline__ bool scalar_target(const float4* __restrict__ pv, const float4* __restrict__ own, const float* __restrict__ sC,
                                              uint32_t idBase, uint32_t n, uint32_t q, float4& P, uint32_t& id, float (&ci)[K]) {
    if (q >= n) return false;
    P = pv[2u * q];
    const float* mine = sC + (size_t)q * (K + 1);
    id = fbits(own[q].w) - idBase;
#pragma unroll
    for (int j = 0; j < K; ++j) ci[j] = mine[j];
    return mine[K] > 0.0f && sample_finite(P.x, P.y, P.z) && P.w > 0.0f && id < n;
}

// The finish of a target and the block's part of the diffusion number (every lane of the block arrives here).
template <int K>
__device__ __forceinline__ void scalar_store(bool target, const ScalarCoef* __restrict__ coef, float kLap, float dt, const float (&ci)[K], const float (&a)[K],
                                             float W, float* __restrict__ c, uint32_t id, uint32_t* __restrict__ state) {
    uint32_t sBits = 0u;
    if (target) {
        const ScalarCoef co = *coef;
        float out[K];
        const float s = scalar_finish<K>(co, kLap, dt, ci, a, W, out);
#pragma unroll
        for (int j = 0; j < K; ++j) c[(size_t)id * K + j] = out[j];
        sBits = fbits(s);
    }
    sBits = wave_max(sBits);                                           // non-negative floats order as their bits: one atomic per wave
    if ((threadIdx.x & 63) == 0 && sBits) atomicMax(&state[0], sBits);
}

// ---- the plain sweep: every candidate from global memory (the bit-level yardstick) ----
template <int K>
__global__ __launch_bounds__(kBlock) void k_scalar_sweep(SimK k, const float4* __restrict__ pv, const float4* __restrict__ own,
                                                         const uint32_t* __restrict__ cellStart, const float* __restrict__ sC,
                                                         const ScalarCoef* __restrict__ coef, float kLap, float dt, float* __restrict__ c,
                                                         uint32_t* __restrict__ state, uint32_t idBase, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t id = 0u;
    float ci[K], a[K], W = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) { ci[j] = 0.0f; a[j] = 0.0f; }
    const bool target = scalar_target<K>(pv, own, sC, idBase, n, q, P, id, ci);
    if (target) {
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int, int, uint32_t qs, uint32_t qe) {
            qe = min(qe, n);                                           // (cellStart never exceeds n; kept so that no load leaves the arrays)
            for (uint32_t j = qs; j < qe; ++j)
                if (j != q) scalar_candidate_global<K>(k, pv, sC, P, ci, j, a, W);
        });
    }
    scalar_store<K>(target, coef, kLap, dt, ci, a, W, c, id, state);
}

// ---- the staged sweep: a block of 256 consecutive slots stages the union of its candidate rows into LDS once ----
// Slots are in cell order, so the block's targets lie in the cells [first slot's cell, last slot's cell] of the linear order.  While
// those are in one z-layer, the candidate rows of all of them are the y-rows [cyA - 1, cyB + 1] of the layers cz - 1 .. cz + 1, whole
// in x (or cx - 1 .. cx + 1 around the block's cells when they are in one y-row).  A staged record is 16 bytes (x, y, z, 1/rho with 0
// for a ghost) plus 4 K bytes of values, 32 KiB per block; a block that spans two z-layers, more than kStageRows rows or more records
// than fit walks global memory.  Same candidate function, same order, therefore the same bits as the plain sweep.
template <int K>
__global__ __launch_bounds__(kBlock) void k_scalar_sweep_staged(SimK k, const float4* __restrict__ pv, const float4* __restrict__ own,
                                                                const uint32_t* __restrict__ cellStart, const float* __restrict__ sC,
                                                                const ScalarCoef* __restrict__ coef, float kLap, float dt, float* __restrict__ c,
                                                                uint32_t* __restrict__ state, uint32_t idBase, uint32_t n) {
    constexpr int CAP = 32768 / (16 + 4 * K);
    __shared__ float4 stP[CAP];
    __shared__ float stC[CAP * K];
    __shared__ uint32_t rowQs[kStageRows], rowOff[kStageRows + 1];
    __shared__ int meta[8];
    const int tid = threadIdx.x;
    const uint32_t q0 = blockIdx.x * kBlock, q = q0 + (uint32_t)tid;
    if (tid < 64) {
        const int lane = tid;
        int staged = 0, rows = 0, cylo = 0, nyS = 0, czlo = 0;
        if (q0 < n) {
            const uint32_t ca = fbits(own[q0].x), cb = fbits(own[min(q0 + (uint32_t)kBlock, n) - 1u].x);
            const int cxa = (int)(ca & 1023u), cya = (int)((ca >> 10) & 1023u), cza = (int)(ca >> 20);
            const int cxb = (int)(cb & 1023u), cyb = (int)((cb >> 10) & 1023u), czb = (int)(cb >> 20);
            cylo = max(cya - 1, 0);
            const int cyhi = min(cyb + 1, k.gy - 1);
            czlo = max(cza - 1, 0);
            const int czhi = min(cza + 1, k.gz - 1);
            nyS = cyhi - cylo + 1;
            rows = nyS * (czhi - czlo + 1);
            const bool oneRow = cya == cyb;
            const int cxlo = oneRow ? max(cxa - 1, 0) : 0, cxhi = oneRow ? min(cxb + 1, k.gx - 1) : k.gx - 1;
            staged = (cza == czb && cza < k.gz && cyb < k.gy && cya <= cyb && cxlo <= cxhi && rows >= 1 && rows <= kStageRows) ? 1 : 0;
            if (staged) {                                              // wave-uniform
                uint32_t qs = 0u, len = 0u;
                if (lane < rows) {
                    const int rowBase = ((czlo + lane / nyS) * k.gy + (cylo + lane % nyS)) * k.gx;
                    qs = cellStart[rowBase + cxlo];
                    len = cellStart[rowBase + cxhi + 1] - qs;
                }
                const uint32_t incl = wave_incl_scan(len);
                const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
                if (lane < rows) { rowQs[lane] = qs; rowOff[lane] = incl - len; }
                if (lane == 0) rowOff[rows] = total;
                staged = total <= (uint32_t)CAP ? 1 : 0;
            }
        }
        if (lane == 0) { meta[0] = staged; meta[1] = rows; meta[2] = cylo; meta[3] = nyS; meta[4] = czlo; }
    }
    __syncthreads();
    const int staged = meta[0];
    if (staged) {                                                      // block-uniform: copy the rows' records into LDS
        const int rows = meta[1];
        const uint32_t total = rowOff[rows];
        for (uint32_t e = (uint32_t)tid; e < total; e += kBlock) {
            int lo = 0, hi = rows - 1;                                 // last row whose offset is <= e
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (rowOff[mid] <= e) lo = mid; else hi = mid - 1; }
            const uint32_t j = min(rowQs[lo] + (e - rowOff[lo]), n - 1u);
            const float4 J = pv[2u * j];
            const float* cj = sC + (size_t)j * (K + 1);
            stP[e] = make_float4(J.x, J.y, J.z, cj[K] > 0.0f ? J.w : 0.0f);
#pragma unroll
            for (int u = 0; u < K; ++u) stC[e * K + u] = cj[u];
        }
    }
    __syncthreads();
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t id = 0u;
    float ci[K], a[K], W = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) { ci[j] = 0.0f; a[j] = 0.0f; }
    const bool target = scalar_target<K>(pv, own, sC, idBase, n, q, P, id, ci);
    if (target) {
        const int rows = meta[1], cylo = meta[2], nyS = meta[3], czlo = meta[4];
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int nz, int ny, uint32_t qs, uint32_t qe) {
            qe = min(qe, n);
            const int sr = (nz - czlo) * nyS + (ny - cylo);
            const bool inRows = staged && nz >= czlo && ny >= cylo && ny < cylo + nyS && sr >= 0 && sr < rows;
            const uint32_t base = inRows ? rowOff[sr] : 0u, first = inRows ? rowQs[sr] : 0u, len = inRows ? rowOff[sr + 1] - base : 0u;
            if (inRows && qs >= first && qe <= first + len) {          // (always when staged, by monotonicity; kept so that LDS is never read outside the rows)
                for (uint32_t j = qs; j < qe; ++j) {
                    if (j == q) continue;
                    const uint32_t e = base + (j - first);
                    const float4 J = stP[e];
                    float cjv[K];
#pragma unroll
                    for (int u = 0; u < K; ++u) cjv[u] = stC[e * K + u];
                    scalar_pair<K>(k.h, k.h2, P.x, P.y, P.z, P.w, ci, J.x, J.y, J.z, J.w, cjv, a, W);
                }
            } else {
                for (uint32_t j = qs; j < qe; ++j)
                    if (j != q) scalar_candidate_global<K>(k, pv, sC, P, ci, j, a, W);
            }
        });
    }
    scalar_store<K>(target, coef, kLap, dt, ci, a, W, c, id, state);
}

// ---- Shepard value of one channel at probe points and on lattices: sum w_j c_jk / sum w_j with the sampler's w_j = ((t t) t) (1/rho_j),
// its candidates and its order (ghost records included, as there); 0 where sum w_j = 0 and for a non-finite point ----
template <int K>
__device__ __forceinline__ float scalar_shepard(const SimK& k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                const float* __restrict__ sC, int channel, float px, float py, float pz) {
    if (!sample_finite(px, py, pz)) return 0.0f;
    float num = 0.0f, wsum = 0.0f;
    const int3 cell = cell_of(k, px, py, pz);
    sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int, int, uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            const float4 J = pv[2u * j];
            const float dx = px - J.x, dy = py - J.y, dz = pz - J.z;
            const float t = fmaxf(k.h2 - dot3(dx, dy, dz, dx, dy, dz), 0.0f);
            const float w = ((t * t) * t) * J.w;
            wsum += w;
            num = fmaf(w, sC[(size_t)j * (K + 1) + channel], num);
        }
    });
    return wsum > 0.0f ? num / wsum : 0.0f;
}
template <int K>
__global__ __launch_bounds__(kBlock) void k_scalar_sample_points(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                                 const float* __restrict__ sC, int channel, const float4* __restrict__ points,
                                                                 float* __restrict__ out, size_t m) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 x = points[i];
    out[i] = scalar_shepard<K>(k, pv, cellStart, sC, channel, x.x, x.y, x.z);
}
// points origin + (float)i * spacing (lattice_coord), x fastest
template <int K>
__global__ __launch_bounds__(kBlock) void k_scalar_sample_lattice(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                                  const float* __restrict__ sC, int channel, float ox, float oy, float oz,
                                                                  float sx, float sy, float sz, int dx, int dy, long long total, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int ix = (int)(i % dx), iy = (int)((i / dx) % dy), iz = (int)(i / ((long long)dx * dy));
        out[i] = scalar_shepard<K>(k, pv, cellStart, sC, channel, lattice_coord(ox, ix, sx), lattice_coord(oy, iy, sy), lattice_coord(oz, iz, sz));
    }
}

// ---- moments: one channel laid out as the statistics kernels' input, so that sph_scalars_moments IS the statistics reduction
// (k_stats_tiles / k_stats_finish: the fixed-order fp64 sums, the extrema with the lowest id).  Per slot q: position record (c, 0, 0, 0),
// velocity record 0, own data with the ghost mark set for every record that is not a target, and the "exact density" c at the slot's
// source index (k_stats_tiles gathers it through order[]).  Then numCounted = targets with a finite value, sumPos[0] = sum c,
// sumDensity2 = sum c c, minPos[0] / maxPos[0] = the extrema. ----
__global__ __launch_bounds__(kBlock) void k_scalar_stat_view(const float4* __restrict__ pv, const float4* __restrict__ own, const uint32_t* __restrict__ order,
                                                             const float* __restrict__ c, int K, int channel, float4* __restrict__ vPv,
                                                             float4* __restrict__ vOwn, float2* __restrict__ vRp, uint32_t idBase, uint32_t n) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const float4 P = pv[2u * q], o = own[q];
    const uint32_t id = fbits(o.w) - idBase;
    const bool target = id < n && !(fbits(o.z) & F_GHOSTNZ) && sample_finite(P.x, P.y, P.z) && P.w > 0.0f;
    const float v = id < n ? c[(size_t)id * K + channel] : 0.0f;
    vPv[2u * q] = make_float4(v, 0.0f, 0.0f, 0.0f);
    vPv[2u * q + 1u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    vOwn[q] = make_float4(o.x, 0.0f, bitsf(target ? 0u : (uint32_t)F_GHOSTNZ), o.w);
    const uint32_t src = order[q];
    if (src < n) vRp[src] = make_float2(v, 0.0f);
}

__global__ __launch_bounds__(kBlock) void k_scalar_seed(const SphParticle* __restrict__ aos, float* __restrict__ c, uint32_t* __restrict__ state, int K, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) state[0] = 0u;
    if (i >= n) return;
    c[(size_t)i * K] = reinterpret_cast<const float*>(aos + i)[15];   // padB
    for (int k = 1; k < K; ++k) c[(size_t)i * K + k] = 0.0f;
}

__global__ void k_scalar_clear_state(uint32_t* __restrict__ state) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) state[0] = 0u;
}

// Strictly inside: dot3(p - centre) < radius * radius (fp32; a non-finite position is never inside).  pos / vel: the internal state
// (slot order, id in vel.w); with pos == nullptr the positions and ghost marks come from the 80-byte records.
__global__ __launch_bounds__(kBlock) void k_scalar_paint(const float4* __restrict__ pos, const float4* __restrict__ vel, const SphParticle* __restrict__ aos,
                                                         float* __restrict__ c, int K, int channel, float cx, float cy, float cz, float r2max,
                                                         float value, int mode, uint32_t idBase, uint32_t n) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    float x, y, z;
    uint32_t id;
    bool ghost;
    if (pos) {
        const float4 P = pos[s];
        x = P.x; y = P.y; z = P.z;
        ghost = (fbits(P.w) & F_GHOSTNZ) != 0u;
        id = fbits(vel[s].w) - idBase;
    } else {
        const float* rec = reinterpret_cast<const float*>(aos + s);
        x = rec[0]; y = rec[1]; z = rec[2];
        ghost = reinterpret_cast<const int*>(rec)[16] != 0;
        id = s;
    }
    if (ghost || id >= n) return;
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    if (!(dot3(dx, dy, dz, dx, dy, dz) < r2max)) return;
    float* d = c + (size_t)id * K + channel;
    *d = mode == kScalarAdd ? *d + value : value;
}

}  // namespace sph
