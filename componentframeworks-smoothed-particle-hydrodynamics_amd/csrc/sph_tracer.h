// sph_tracer.h -- passive tracers advected inside the substep, with pathlines (no reference counterpart).
//
// A tracer is a point the fluid carries.  Every substep moves it with the Shepard velocity u(x) of sph_sample.h, evaluated on the
// sorted copy of the substep's ENTRY state (the grid dispatch_one has just built for the SPH pass), per axis with an fp32 multiply
// and then an add (-ffp-contract=off: no fma):
//   Euler     v = u(x);                                   x' = x + dt * v
//   midpoint  v1 = u(x); xm = x + (0.5f * dt) * v1; v = u(xm); x' = x + dt * v
// and stores vel = v, fraction = phi(x) at the position BEFORE the move, age' = age + dt.  A non-finite tracer keeps its position
// bits, gets vel = fraction = 0 and still ages.  u() is sample_rows / sample_candidate / sample_finish
// of the sampler itself: a tracer is, bit for bit, a probe of sph_sample_points that the host moved.
//
//   k_tracer_seed     points (x, y, z, age) -> 32-byte records, identity processing order, snapshot 0, step counter 0
//   k_tracer_advect   one tracer per lane in PROCESSING order (perm[]): lanes of a wave then share candidate rows once perm[] is
//                     cell-sorted; the record is read and written at its caller-order index, so no result depends on perm[]
//   k_tracer_tick     one thread behind k_tracer_advect: step counter += 1 and the ring slot of the NEXT substep's snapshot
//                     (device memory, because a captured graph bakes its launch arguments in)
//   k_tracer_bin / k_tracer_scatter   counting sort of the tracers by cell (with the engine's scan kernels in between): perm[]
#pragma once
#include "sph_sample.h"

namespace sph {

constexpr uint32_t kTracerNoSlot = 0xFFFFFFFFu;
#ifndef SPH_TRACER_REFRESH
#define SPH_TRACER_REFRESH 8       // substeps between two cell sorts of the processing order (bits do not depend on it)
#endif
constexpr int kTracerRefresh = SPH_TRACER_REFRESH;
constexpr int kTracerAhead = 4;             // candidates whose records are in flight before the first of them is accumulated

// state[0], state[1]: low / high word of the substeps c that advected this tracer set; state[2]: ring slot substep c + 1 writes, or none
__host__ __device__ __forceinline__ uint32_t tracer_slot_of(unsigned long long c, uint32_t K, uint32_t S) {
    return (K != 0u && c % S == 0ull) ? (uint32_t)((c / S) % K) : kTracerNoSlot;
}

__global__ __launch_bounds__(kBlock) void k_tracer_seed(const float4* __restrict__ points, float4* __restrict__ rec, uint32_t* __restrict__ perm,
                                                        float4* __restrict__ ring, uint32_t* __restrict__ state, uint32_t m, uint32_t K, uint32_t S) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) { state[0] = 0u; state[1] = 0u; state[2] = tracer_slot_of(1ull, K, S); }
    if (i >= m) return;
    const float4 p = points[i];
    rec[2u * i] = p;
    rec[2u * i + 1u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    perm[i] = i;
    if (K) ring[i] = p;                                                // snapshot 0 is the seed
}

__device__ __forceinline__ SampleOut tracer_field(const SimK& k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                  float x, float y, float z) {
    SampleOut o{};
    if (!sample_finite(x, y, z)) return o;
    // (sample_ahead of sph_sample.h: the loads of kTracerAhead candidates in flight at once, the bits of sample_global)
    return sample_finish(k, sample_ahead<kTracerAhead>(k, pv, cellStart, x, y, z));
}

template <bool MIDPOINT>
__global__ __launch_bounds__(kBlock) void k_tracer_advect(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart, float dt,
                                                          const uint32_t* __restrict__ perm, float4* __restrict__ rec, float4* __restrict__ ring,
                                                          const uint32_t* __restrict__ state, uint32_t m) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = perm[t];
    if (i >= m) return;                                                // (never: perm[] is a permutation of [0, m))
    float4 a = rec[2u * i];
    float vx = 0.0f, vy = 0.0f, vz = 0.0f, fraction = 0.0f;
    if (sample_finite(a.x, a.y, a.z)) {
        SampleOut o = tracer_field(k, pv, cellStart, a.x, a.y, a.z);
        fraction = o.fraction;
        if (MIDPOINT) {
            const float hd = 0.5f * dt;
            o = tracer_field(k, pv, cellStart, a.x + hd * o.vx, a.y + hd * o.vy, a.z + hd * o.vz);
        }
        vx = o.vx; vy = o.vy; vz = o.vz;
        a.x = a.x + dt * vx; a.y = a.y + dt * vy; a.z = a.z + dt * vz;
    }
    a.w = a.w + dt;
    rec[2u * i] = a;
    rec[2u * i + 1u] = make_float4(vx, vy, vz, fraction);
    const uint32_t slot = state[2];
    if (slot != kTracerNoSlot) ring[(size_t)slot * m + i] = a;
}

__global__ void k_tracer_tick(uint32_t* __restrict__ state, uint32_t K, uint32_t S) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const unsigned long long c = (((unsigned long long)state[1] << 32) | state[0]) + 1ull;
    state[0] = (uint32_t)c; state[1] = (uint32_t)(c >> 32);
    state[2] = tracer_slot_of(c + 1ull, K, S);
}

// ---- processing order: tracers sorted by cell (arrival order inside a cell is arbitrary; nothing depends on it) ----
__global__ __launch_bounds__(kBlock) void k_tracer_bin(SimK k, const float4* __restrict__ rec, uint2* __restrict__ key, uint32_t* __restrict__ cellCount, uint32_t m) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 p = rec[2u * i];
    // (cell_axis clamps: a tracer outside the grid or with a non-finite coordinate still lands in [0, numCells))
    const int3 c = cell_of(k, p.x, p.y, p.z);
    const uint32_t cell = (uint32_t)((c.z * k.gy + c.y) * k.gx + c.x);
    key[i] = make_uint2(cell, atomicAdd(&cellCount[cell], 1u));
}

__global__ __launch_bounds__(kBlock) void k_tracer_scatter(const uint2* __restrict__ key, const uint32_t* __restrict__ cellStart, uint32_t* __restrict__ perm, uint32_t m) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint2 q = key[i];
    const uint32_t s = cellStart[q.x] + q.y;
    if (s < m) perm[s] = i;
}

}  // namespace sph
