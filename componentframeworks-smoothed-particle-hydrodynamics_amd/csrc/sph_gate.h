// sph_gate.h -- flow gates: what crosses an oriented planar patch, counted inside the substep (no reference counterpart).
//
// A gate is a rectangle or an ellipse fixed in the world: centre c and two half-extent vectors u, v; the forward normal is N = cross(u, v),
// not normalised.  One step, on the OUTPUT state of the substep (slot order, id in vel.w), after the container, the obstacle step and the
// coupling step and before river / fountain.  After the SPH pass slot s of the sorted copy holds the ENTRY state of the particle whose
// exit state the pass wrote to slot s of the output arrays, so a crossing is decided from two loads at the same index:
//
//   side     s0 = dot3(p0 - c, N), s1 = dot3(p1 - c, N); forward s0 < 0 && s1 >= 0, backward s0 >= 0 && s1 < 0 (a NaN is no crossing)
//   where    t = s0 / (s0 - s1), x_a = fmaf(t, p1_a - p0_a, p0_a), d = x - c, a = dot3(d, u), b = dot3(d, v); rectangle |a| < u.u && |b| < v.v;
//            ellipse fmaf(fa, fa, fb * fb) < 1 with fa = a / u.u, fb = b / v.v; GATE_UNBOUNDED: the whole plane
//   books    per gate the forward and backward counts and the fp64 sums of +-(double)v_a and +-(double)c_k over the counted crossers
//
// gate_normal / gate_side / gate_counts are __host__ __device__: sph_gates_step_host runs the same functions in a plain loop.
// fp32, every operation rounded on its own except dot3 and the explicit fmaf (-ffp-contract=off).
//
//   k_gates<K>        sweeps over the output slots with a FIXED grid and the sweep / unroll shape of k_obstacles (the constants are
//                     restated here: a feature header includes no other feature): loads pos[s] and sPV[2 s]; per gate the lane tests the
//                     sign change and the wave skips the gate where no lane crosses; vel[s] and c[id K ..] are loaded by crossing lanes
//                     only.  Per wave an xor butterfly of every fp64 term that lane 0 adds to its wave's LDS row; one partial row per
//                     block (its waves in order).  It writes no particle state.
//   k_gates_finish    one block: the partial rows summed in a fixed order (contiguous ranges, each ascending, then the ranges in order) into
//                     the books, time += dt, substeps += 1, and every `stride` substeps the cumulative books and the time into a ring row.
// The gate table, the count, the ring's length and stride live in device memory (GateTab), never in launch arguments, so a replayed graph
// sees every later sph_gates_set.  No float atomic is used: the sums depend on the slot order only.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_kernels.h"

namespace sph {

constexpr int kGateMax = 8;                            // SPH_MAX_GATES
constexpr int kGateBlock = 512;                        // threads per block of k_gates (the sweep of k_obstacles, restated)
constexpr int kGateUnroll = 2;                         // slots per thread and sweep, their loads issued together
constexpr int kGateSweep = kGateBlock * kGateUnroll;
constexpr int kGateGrid = 1024;                        // blocks of k_gates at most: rows of the partial slab
constexpr int kGateWaves = kGateBlock / 64;
constexpr int kGateChannels = 4;                       // SPH_MAX_SCALAR_CHANNELS
constexpr int kGateSums = 3 + kGateChannels;           // fp64 sums per gate: vel[3], scalar[4]
constexpr int kGateWords = 2 + kGateSums;              // 8-byte words per gate: forward, backward, then the sums (the layout of SphGateBooks)
constexpr int kGateTerms = kGateMax * kGateWords;      // 8-byte words per partial row, per books table and per ring row
constexpr int kGateRingRow = kGateTerms + 1;           // a ring row: the books of every gate, then the time
constexpr int kGateHistoryMax = 4096;
constexpr int kGateFinishBlock = 1024;                 // threads of k_gates_finish
enum : int32_t { GATE_RECT = 0, GATE_ELLIPSE = 1 };    // SPH_GATE_RECT / SPH_GATE_ELLIPSE
enum : int32_t { GATE_UNBOUNDED = 1 };                 // SPH_GATE_UNBOUNDED

// One gate as the kernel reads it: SphGate (64 bytes) with the derived values in its padding.
struct GateRec {
    int32_t shape, flags;
    float c[3];
    float u[3], v[3];
    float N[3];                                        // gate_normal(u, v)
    float uu, vv;                                      // dot3(u, u), dot3(v, v)
};
static_assert(sizeof(GateRec) == 64, "GateRec must be 64 bytes");

// What the kernels read, in DEVICE memory.
struct GateTab {
    int32_t count;
    uint32_t history, stride;                          // ring rows (0: none) and substeps per row
    int32_t pad;
    GateRec g[kGateMax];
};
static_assert(sizeof(GateTab) == 16 + 64 * kGateMax, "GateTab layout");

struct GateAcc {
    unsigned long long words[kGateTerms];              // SphGateBooks[kGateMax]: two counts, then seven doubles, per gate
    double time;                                       // fp64 sum of dt since the books were last zeroed
    unsigned long long substeps;                       // substeps since then
    unsigned long long ringSteps;                      // substeps since the ring was last zeroed
};

// N = cross(u, v): per component a multiply, a multiply and a subtract.
__host__ __device__ inline void gate_normal(const float* u, const float* v, float* N) {
    N[0] = u[1] * v[2] - u[2] * v[1];
    N[1] = u[2] * v[0] - u[0] * v[2];
    N[2] = u[0] * v[1] - u[1] * v[0];
}
// The derived values of a gate from its centre and half-extent vectors.
__host__ __device__ inline void gate_derive(GateRec& G) {
    gate_normal(G.u, G.v, G.N);
    G.uu = dot3(G.u[0], G.u[1], G.u[2], G.u[0], G.u[1], G.u[2]);
    G.vv = dot3(G.v[0], G.v[1], G.v[2], G.v[0], G.v[1], G.v[2]);
}
// Signed (unnormalised) distance of a point from the gate's plane.
__host__ __device__ inline float gate_side(const GateRec& G, float px, float py, float pz) {
    return dot3(px - G.c[0], py - G.c[1], pz - G.c[2], G.N[0], G.N[1], G.N[2]);
}
// +1 forward, -1 backward, 0 no crossing (a NaN compares false).
__host__ __device__ inline int gate_crossing(float s0, float s1) {
    if (s0 < 0.0f && s1 >= 0.0f) return 1;
    if (s0 >= 0.0f && s1 < 0.0f) return -1;
    return 0;
}
// Does the segment p0 -> p1 (sides s0, s1 of a crossing) meet the plane inside the patch?
__host__ __device__ inline bool gate_counts(const GateRec& G, float p0x, float p0y, float p0z, float p1x, float p1y, float p1z, float s0, float s1) {
    if (G.flags & GATE_UNBOUNDED) return true;
    const float t = s0 / (s0 - s1);
    const float dx = fmaf(t, p1x - p0x, p0x) - G.c[0], dy = fmaf(t, p1y - p0y, p0y) - G.c[1], dz = fmaf(t, p1z - p0z, p0z) - G.c[2];
    const float a = dot3(dx, dy, dz, G.u[0], G.u[1], G.u[2]), b = dot3(dx, dy, dz, G.v[0], G.v[1], G.v[2]);
    if (G.shape == GATE_ELLIPSE) {
        const float fa = a / G.uu, fb = b / G.vv;
        return fmaf(fa, fa, fb * fb) < 1.0f;
    }
    return fabsf(a) < G.uu && fabsf(b) < G.vv;
}

// One slot against gates 0 .. count-1.  P1 / P0: the exit and the entry position of the slot (P1.w: the flags).  cand: s < n, no ghost or
// halo bit, both positions finite.  vel and c are read by crossing lanes only; a crosser whose id is not one of the engine's is not booked.
template <int K>
__device__ __forceinline__ void gate_slot(const GateTab* __restrict__ tab, int count, const float4* __restrict__ vel, const float* __restrict__ c,
                                          uint32_t idBase, int n, int s, float4 P1, float4 P0, bool cand, double* rowSum, unsigned long long* rowCnt,
                                          int lane) {
    bool haveV = false, idOk = false;
    float4 V = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float cv[K > 0 ? K : 1] = {0.0f};
    bool haveC = false;
    uint32_t id = 0u;
    for (int g = 0; g < count; ++g) {
        const GateRec& G = tab->g[g];                                  // (wave-uniform addresses)
        const float s0 = gate_side(G, P0.x, P0.y, P0.z), s1 = gate_side(G, P1.x, P1.y, P1.z);
        const int dir = cand ? gate_crossing(s0, s1) : 0;
        if (__ballot(dir != 0) == 0ull) continue;                      // (wave-uniform)
        if (dir != 0 && !haveV) {
            V = vel[s];
            id = fbits(V.w) - idBase;
            idOk = id < (uint32_t)n;
            haveV = true;
        }
        const bool counted = dir != 0 && idOk && gate_counts(G, P0.x, P0.y, P0.z, P1.x, P1.y, P1.z, s0, s1);
        const unsigned long long fw = __ballot(counted && dir > 0), bw = __ballot(counted && dir < 0);
        if ((fw | bw) == 0ull) continue;                               // (wave-uniform: every term is +0.0)
        double t[3 + K];
#pragma unroll
        for (int j = 0; j < 3 + K; ++j) t[j] = 0.0;
        if (counted) {
            const double sg = dir > 0 ? 1.0 : -1.0;
            t[0] = sg * (double)V.x; t[1] = sg * (double)V.y; t[2] = sg * (double)V.z;
            if constexpr (K > 0) {
                if (!haveC) {
#pragma unroll
                    for (int k = 0; k < K; ++k) cv[k] = c[(size_t)id * K + k];
                    haveC = true;
                }
#pragma unroll
                for (int k = 0; k < K; ++k) t[3 + k] = float_finite(cv[k]) ? sg * (double)cv[k] : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < 3 + K; ++j) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) t[j] += __shfl_xor(t[j], o, 64);
        }
        if (lane == 0) {
            rowCnt[2 * g] += (unsigned long long)__popcll(fw);
            rowCnt[2 * g + 1] += (unsigned long long)__popcll(bw);
#pragma unroll
            for (int j = 0; j < 3 + K; ++j) rowSum[kGateSums * g + j] += t[j];
        }
    }
}

// Sweeps of kGateSweep slots: slot base + j kGateBlock + thread for j = 0 .. kGateUnroll - 1, the loads of the kGateUnroll slots issued
// together.  sPV: the sorted copy of the entry state (two float4 per slot, the position first).  part: rows of kGateTerms 8-byte words in
// the layout of the books.
template <int K>
__global__ __launch_bounds__(kGateBlock) void k_gates(const GateTab* __restrict__ tab, const float4* __restrict__ pos, const float4* __restrict__ vel,
                                                      const float4* __restrict__ sPV, const float* __restrict__ c, uint32_t idBase, int n,
                                                      unsigned long long* __restrict__ part) {
    __shared__ double ssum[kGateWaves][kGateMax * kGateSums];
    __shared__ unsigned long long scnt[kGateWaves][kGateMax * 2];
    const int count = min(max(tab->count, 0), kGateMax);
    for (int i = threadIdx.x; i < kGateWaves * kGateMax * kGateSums; i += kGateBlock) (&ssum[0][0])[i] = 0.0;
    if (threadIdx.x < kGateWaves * kGateMax * 2) (&scnt[0][0])[threadIdx.x] = 0ull;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int base = blockIdx.x * kGateSweep; base < n; base += gridDim.x * kGateSweep) {     // (block-uniform)
        float4 P1[kGateUnroll], P0[kGateUnroll];
#pragma unroll
        for (int j = 0; j < kGateUnroll; ++j) {
            const int s = base + j * kGateBlock + threadIdx.x;
            P1[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            P0[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < n) { P1[j] = pos[s]; P0[j] = sPV[2 * (size_t)s]; }
        }
#pragma unroll
        for (int j = 0; j < kGateUnroll; ++j) {
            const int s = base + j * kGateBlock + threadIdx.x;
            const bool cand = s < n && !(fbits(P1[j].w) & (F_GHOSTNZ | F_HALO)) && float_finite(P1[j].x) && float_finite(P1[j].y) && float_finite(P1[j].z) &&
                              float_finite(P0[j].x) && float_finite(P0[j].y) && float_finite(P0[j].z);
            gate_slot<K>(tab, count, vel, c, idBase, n, s, P1[j], P0[j], cand, ssum[wave], scnt[wave], lane);
        }
    }
    __syncthreads();
    if (threadIdx.x < kGateTerms) {
        const int g = threadIdx.x / kGateWords, j = threadIdx.x % kGateWords;
        unsigned long long word;
        if (j < 2) {
            word = 0ull;
            for (int w = 0; w < kGateWaves; ++w) word += scnt[w][2 * g + j];
        } else {
            double r = ssum[0][kGateSums * g + (j - 2)];
            for (int w = 1; w < kGateWaves; ++w) r += ssum[w][kGateSums * g + (j - 2)];
            word = (unsigned long long)__double_as_longlong(r);
        }
        part[(size_t)blockIdx.x * kGateTerms + threadIdx.x] = word;
    }
}

// One block.  The rows are cut into chunks = min(kGateFinishBlock / kGateTerms, rows) contiguous ranges of ceil(rows / chunks); thread
// (chunk, term) sums its range in ascending row order, then thread `term` sums the chunk sums in chunk order and adds the result to the
// books.  Then the ring: when the substeps since the ring was zeroed reach a multiple of the stride, the books and the time go into row
// (substeps / stride - 1) mod history (ringCap: the rows the ring buffer has room for).
__global__ __launch_bounds__(kGateFinishBlock) void k_gates_finish(float dt, const unsigned long long* __restrict__ part, int rows,
                                                                  const GateTab* __restrict__ tab, GateAcc* __restrict__ acc,
                                                                  unsigned long long* __restrict__ ring, uint32_t ringCap) {
    __shared__ unsigned long long sums[kGateFinishBlock];
    __shared__ unsigned long long sStep;
    __shared__ double sTime;
    constexpr int kChunksMax = kGateFinishBlock / kGateTerms;
    const int chunks = max(1, min(kChunksMax, rows));
    const int t = threadIdx.x, term = t % kGateTerms, ch = t / kGateTerms;
    const bool isCount = term % kGateWords < 2;
    if (ch < chunks && ch < kChunksMax) {
        const int per = (rows + chunks - 1) / chunks;
        const int r1 = min(rows, (ch + 1) * per);
        if (isCount) {
            unsigned long long s = 0ull;
            for (int r = ch * per; r < r1; ++r) s += part[(size_t)r * kGateTerms + term];
            sums[ch * kGateTerms + term] = s;
        } else {
            double s = 0.0;
            for (int r = ch * per; r < r1; ++r) s += __longlong_as_double((long long)part[(size_t)r * kGateTerms + term]);
            sums[ch * kGateTerms + term] = (unsigned long long)__double_as_longlong(s);
        }
    }
    if (t == 0) {
        sTime = acc->time + (double)dt;
        acc->time = sTime;
        acc->substeps += 1ull;
        sStep = acc->ringSteps + 1ull;
        acc->ringSteps = sStep;
    }
    __syncthreads();
    const uint32_t H = min(tab->history, ringCap), S = max(tab->stride, 1u);
    const bool store = H > 0u && sStep % S == 0ull;
    const size_t row = store ? (size_t)((sStep / S - 1ull) % H) : 0;
    if (t < kGateTerms) {
        unsigned long long word;
        if (isCount) {
            unsigned long long s = 0ull;
            for (int k = 0; k < chunks; ++k) s += sums[k * kGateTerms + t];
            word = acc->words[t] + s;
        } else {
            double s = __longlong_as_double((long long)sums[t]);
            for (int k = 1; k < chunks; ++k) s += __longlong_as_double((long long)sums[k * kGateTerms + t]);
            word = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)acc->words[t]) + s);
        }
        acc->words[t] = word;
        if (store) ring[row * kGateRingRow + t] = word;
    }
    if (t == 0 && store) ring[row * kGateRingRow + kGateTerms] = (unsigned long long)__double_as_longlong(sTime);
}
}  // namespace sph
