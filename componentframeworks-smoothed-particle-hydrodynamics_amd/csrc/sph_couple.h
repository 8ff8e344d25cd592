// sph_couple.h -- active scalars: buoyancy from the channels and continuous sources / sinks (no reference counterpart).
//
// The scalar channels of sph_scalar.h act back on the fluid and are fed every substep on the device.  One step, on the OUTPUT state of the
// substep (slot order, id in vel.w), after the container and the obstacle step and before river / fountain:
//
//   sources    0 .. S-1 in order, each on the result of the ones before it: a target strictly inside the region (a sphere or a box, in
//              the world frame or in the local frame of obstacle `body`, read from the device ObsRec: the pose AFTER this substep's
//              obstacle step) whose value in the source's channel is finite gets c' = c + dt rate (RATE) or
//              c' = c + fminf(dt rate, 1) (target - c), clamped between c and target (RELAX).  Per source the hits and the fp64 sum of (double)c' - (double)c are kept.
//   buoyancy   s = fmaf(beta_k, c_k - ref_k, s) over the channels (the values the sources just wrote); where s is finite and != 0,
//              v_a' = v_a - (dt s) g_a.  Positions are not touched, the velocity is not capped.
//
// couple_inside / couple_apply / couple_kick are __host__ __device__: sph_scalars_couple_host runs the same functions in a plain loop.
// fp32, every operation rounded on its own except the explicit fmaf()s (-ffp-contract=off).
//
//   k_scalar_couple<K, SRC, BUOY>   sweeps over the output slots with the FIXED grid and the sweep / unroll shape of k_obstacles: loads
//                       pos and vel (the id is vel.w), gathers c[id K ..], tests the sources behind a per-wave world-AABB cull (the boxes
//                       are built once per block into LDS; the exact test reads the source and its body at wave-uniform addresses), writes
//                       c only where a source hit and vel only where the kick changed it.  Per wave an xor butterfly of each source's fp64
//                       term that lane 0 adds to its wave's LDS row; one partial row per block (its waves in order).
//   k_scalar_couple_finish   one block (SRC only): the partial rows summed in a fixed order (contiguous ranges, each ascending, then the
//                       ranges in order) into the books, time += dt, substeps += 1.
// The coefficients, the source table and the source count live in device memory (CoupleTab), never in launch arguments, so a replayed
// graph sees every later sph_scalars_set_buoyancy / _set_sources.  No float atomic is used: the sums depend on the slot order only.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_obstacle.h"   // built on it: a source may sit in a body's frame (ObsRec), and the sweep has k_obstacles' shape (kObs*)
#include "sph_scalar.h"     // built on it: the channels it acts on (kScalarMax)

namespace sph {

constexpr int kCoupleMax = 8;                          // SPH_MAX_SCALAR_SOURCES
constexpr int kCoupleFinishBlock = 1024;               // threads of k_scalar_couple_finish
constexpr int kCoupleTerms = 2 * kCoupleMax;           // per partial row: the sums, then the hits
enum : int32_t { COUPLE_SPHERE = 0, COUPLE_BOX = 1 };  // SPH_SOURCE_SPHERE / SPH_SOURCE_BOX
enum : int32_t { COUPLE_RATE = 0, COUPLE_RELAX = 1 };  // SPH_SOURCE_RATE / SPH_SOURCE_RELAX

// One source: the layout of SphScalarSource (64 bytes).
struct CoupleSrc {
    int32_t shape, channel, mode, body;
    float center[3];
    float size[3];
    float rate, target;
    float pad[4];
};
static_assert(sizeof(CoupleSrc) == 64, "CoupleSrc must be 64 bytes");

// What the kernel reads, in DEVICE memory.
struct CoupleTab {
    float beta[kScalarMax];
    float ref[kScalarMax];
    int32_t nSrc;
    int32_t pad[3];
    CoupleSrc src[kCoupleMax];
};
static_assert(sizeof(CoupleTab) == 48 + 64 * kCoupleMax, "CoupleTab layout");

struct CoupleAcc {
    double sum[kCoupleMax];                            // fp64 sum of (double)c' - (double)c per source
    unsigned long long hits[kCoupleMax];               // (particle, substep) hits per source
    double time;                                       // fp64 sum of dt
    unsigned long long substeps;
};

// Strictly inside?  B: the body of a body-bound source (nullptr: the world frame).  A non-finite coordinate is never inside.
__host__ __device__ inline bool couple_inside(const CoupleSrc& S, const ObsRec* B, float px, float py, float pz) {
    float dx, dy, dz;
    if (B) {
        const float qx = px - B->c[0], qy = py - B->c[1], qz = pz - B->c[2];
        const float* M = B->M;
        dx = dot3(qx, qy, qz, M[0], M[3], M[6]) - S.center[0];   // l = M^T (p - c_b), d = l - center
        dy = dot3(qx, qy, qz, M[1], M[4], M[7]) - S.center[1];
        dz = dot3(qx, qy, qz, M[2], M[5], M[8]) - S.center[2];
    } else {
        dx = px - S.center[0]; dy = py - S.center[1]; dz = pz - S.center[2];
    }
    if (S.shape == COUPLE_SPHERE) return dot3(dx, dy, dz, dx, dy, dz) < S.size[0] * S.size[0];
    return fabsf(dx) < S.size[0] && fabsf(dy) < S.size[1] && fabsf(dz) < S.size[2];
}

// The new value of a hit: a multiply and then an add, no fma.  RELAX: with a = 1 (or within a rounding of it) the sum c + (target - c)
// can miss the target by a rounding of the subtraction, on either side (c = 1, target = 0.3f), so the result is clamped into the closed
// interval between c and target: it never leaves it, whatever dt rate is.
__host__ __device__ inline float couple_apply(const CoupleSrc& S, float dt, float c) {
    if (S.mode == COUPLE_RATE) return c + dt * S.rate;
    const float a = fminf(dt * S.rate, 1.0f);
    const float r = c + a * (S.target - c);
    return fminf(fmaxf(r, fminf(c, S.target)), fmaxf(c, S.target));
}

// The buoyancy kick of one record; false (nothing to write) where s is not finite or zero.
template <int K>
__host__ __device__ inline bool couple_kick(const float* beta, const float* ref, const float (&c)[K], float dt, float gx, float gy, float gz,
                                            float& vx, float& vy, float& vz) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) s = fmaf(beta[k], c[k] - ref[k], s);
    if (!float_finite(s) || s == 0.0f) return false;
    const float f = dt * s;
    vx = vx - f * gx; vy = vy - f * gy; vz = vz - f * gz;
    return true;
}

// World AABB of a source for the per-wave cull: centre and half extents with a margin far above the rounding of the exact test
// (relative 1e-3 of the extent, and 1e-5 of every length that enters the body-frame transform).  A cull only: it never changes a result.
struct CoupleBox { float c[3], e[3]; };
__host__ __device__ inline void couple_box(const CoupleSrc& S, const ObsRec* B, CoupleBox& X) {
    float mag = fabsf(S.center[0]) + fabsf(S.center[1]) + fabsf(S.center[2]) + S.size[0] + (S.shape == COUPLE_BOX ? S.size[1] + S.size[2] : 0.0f);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float e;
        if (B) {
            const float* m = B->M + 3 * a;
            X.c[a] = B->c[a] + (m[0] * S.center[0] + m[1] * S.center[1] + m[2] * S.center[2]);
            e = S.shape == COUPLE_SPHERE ? S.size[0] : fabsf(m[0]) * S.size[0] + fabsf(m[1]) * S.size[1] + fabsf(m[2]) * S.size[2];
        } else {
            X.c[a] = S.center[a];
            e = S.shape == COUPLE_SPHERE ? S.size[0] : S.size[a];
        }
        X.e[a] = e;
    }
    if (B) mag += fabsf(B->c[0]) + fabsf(B->c[1]) + fabsf(B->c[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        X.e[a] = X.e[a] * 1.001f + 1e-6f + 1e-5f * mag;
        if (!(X.e[a] >= 0.0f) || !float_finite(X.c[a])) X.e[a] = INFINITY;   // (a box that cannot be formed culls nothing)
    }
}

// One slot against sources 0 .. S-1 in order, then the kick.  bodies / nBodies: the obstacle set (a source whose body is not in it is
// skipped; the host refuses such a dispatch before it is enqueued).
template <int K, bool SRC, bool BUOY>
__device__ __forceinline__ void couple_slot(const CoupleTab* __restrict__ tab, const ObsRec* __restrict__ bodies, int nBodies, int nSrc,
                                            const CoupleBox* boxes, float dt, float gx, float gy, float gz, float4* __restrict__ vel,
                                            float* __restrict__ c, int s, float4 P, float4 V, uint32_t id, bool cand, double* rowSum,
                                            unsigned long long* rowHits, int lane) {
    float cv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cv[k] = 0.0f;
    if (cand) {
#pragma unroll
        for (int k = 0; k < K; ++k) cv[k] = c[(size_t)id * K + k];
    }
    if constexpr (SRC) {
        bool wrote = false;
        for (int i = 0; i < nSrc; ++i) {
            const CoupleBox& X = boxes[i];
            const bool near = cand && fabsf(P.x - X.c[0]) <= X.e[0] && fabsf(P.y - X.c[1]) <= X.e[1] && fabsf(P.z - X.c[2]) <= X.e[2];
            if (__ballot(near) == 0ull) continue;                     // (wave-uniform)
            const CoupleSrc& S = tab->src[i];                         // (wave-uniform addresses)
            const int body = S.body;
            if (body >= nBodies) continue;
            const ObsRec* B = body >= 0 ? bodies + body : nullptr;
            double t = 0.0;
            bool hit = false;
            if (near && couple_inside(S, B, P.x, P.y, P.z)) {
                const int ch = S.channel;
                float old = 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) if (k == ch) old = cv[k];
                if (float_finite(old) && ch >= 0 && ch < K) {
                    const float now = couple_apply(S, dt, old);
#pragma unroll
                    for (int k = 0; k < K; ++k) if (k == ch) cv[k] = now;
                    t = (double)now - (double)old;
                    hit = true;
                    wrote = true;
                }
            }
            const unsigned long long h = (unsigned long long)__popcll(__ballot(hit));
            if (h == 0ull) continue;                                  // (wave-uniform: every term is +0.0)
            t = wave_sum(t);
            if (lane == 0) { rowSum[i] += t; rowHits[i] += h; }
        }
        if (wrote) {
#pragma unroll
            for (int k = 0; k < K; ++k) c[(size_t)id * K + k] = cv[k];
        }
    }
    if constexpr (BUOY) {
        if (cand && couple_kick<K>(tab->beta, tab->ref, cv, dt, gx, gy, gz, V.x, V.y, V.z)) vel[s] = V;
    }
}

// Sweeps of kObsSweep slots, as k_obstacles: slot base + j kObsBlock + thread for j = 0 .. kObsUnroll - 1, the loads of the kObsUnroll
// slots issued together.  part: rows of kCoupleTerms 8-byte words (the sums as doubles, then the hits as unsigned 64-bit integers).
template <int K, bool SRC, bool BUOY>
__global__ __launch_bounds__(kObsBlock) void k_scalar_couple(const CoupleTab* __restrict__ tab, const ObsRec* __restrict__ bodies, int nBodies, float dt,
                                                             float gx, float gy, float gz, const float4* __restrict__ pos, float4* __restrict__ vel,
                                                             float* __restrict__ c, uint32_t idBase, int n, double* __restrict__ part) {
    __shared__ double ssum[kObsWaves][kCoupleMax];
    __shared__ unsigned long long shits[kObsWaves][kCoupleMax];
    __shared__ CoupleBox boxes[kCoupleMax];
    int nSrc = 0;
    if constexpr (SRC) {
        nSrc = min(max(tab->nSrc, 0), kCoupleMax);
        if (threadIdx.x < kObsWaves * kCoupleMax) { (&ssum[0][0])[threadIdx.x] = 0.0; (&shits[0][0])[threadIdx.x] = 0ull; }
        if ((int)threadIdx.x < nSrc) {
            const CoupleSrc& S = tab->src[threadIdx.x];
            const int body = S.body;
            couple_box(S, (body >= 0 && body < nBodies) ? bodies + body : nullptr, boxes[threadIdx.x]);
        }
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int base = blockIdx.x * kObsSweep; base < n; base += gridDim.x * kObsSweep) {     // (block-uniform)
        float4 P[kObsUnroll], V[kObsUnroll];
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            P[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            V[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < n) { P[j] = pos[s]; V[j] = vel[s]; }
        }
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            const uint32_t id = fbits(V[j].w) - idBase;
            const bool cand = s < n && id < (uint32_t)n && !(fbits(P[j].w) & (F_GHOSTNZ | F_HALO)) && float_finite(P[j].x) && float_finite(P[j].y) &&
                              float_finite(P[j].z);
            couple_slot<K, SRC, BUOY>(tab, bodies, nBodies, nSrc, boxes, dt, gx, gy, gz, vel, c, s, P[j], V[j], id, cand, ssum[wave], shits[wave], lane);
        }
    }
    if constexpr (SRC) {
        __syncthreads();
        if (threadIdx.x < kCoupleMax) {
            double r = ssum[0][threadIdx.x];
            for (int w = 1; w < kObsWaves; ++w) r += ssum[w][threadIdx.x];
            part[(size_t)blockIdx.x * kCoupleTerms + threadIdx.x] = r;
        } else if (threadIdx.x < kCoupleTerms) {
            const int i = threadIdx.x - kCoupleMax;
            unsigned long long r = 0ull;
            for (int w = 0; w < kObsWaves; ++w) r += shits[w][i];
            reinterpret_cast<unsigned long long*>(part)[(size_t)blockIdx.x * kCoupleTerms + threadIdx.x] = r;
        }
    }
}

// One block.  The rows are cut into chunks = min(kCoupleFinishBlock / kCoupleTerms, rows) contiguous ranges of ceil(rows / chunks); thread
// (chunk, term) sums its range in ascending row order, then thread `term` sums the chunk sums in chunk order and adds the result to the books.
__global__ __launch_bounds__(kCoupleFinishBlock) void k_scalar_couple_finish(float dt, const double* __restrict__ part, int rows, CoupleAcc* __restrict__ acc) {
    __shared__ double sums[kCoupleFinishBlock];
    __shared__ unsigned long long cnts[kCoupleFinishBlock];
    const int chunks = max(1, min(kCoupleFinishBlock / kCoupleTerms, rows));
    const int t = threadIdx.x, term = t % kCoupleTerms, ch = t / kCoupleTerms;
    if (ch < chunks) {
        const int per = (rows + chunks - 1) / chunks;
        const int r1 = min(rows, (ch + 1) * per);
        if (term < kCoupleMax) {
            double s = 0.0;
            for (int r = ch * per; r < r1; ++r) s += part[(size_t)r * kCoupleTerms + term];
            sums[ch * kCoupleTerms + term] = s;
        } else {
            const unsigned long long* hp = reinterpret_cast<const unsigned long long*>(part);
            unsigned long long s = 0ull;
            for (int r = ch * per; r < r1; ++r) s += hp[(size_t)r * kCoupleTerms + term];
            cnts[ch * kCoupleTerms + term] = s;
        }
    }
    __syncthreads();
    if (t < kCoupleMax) {
        double s = sums[t];
        for (int k = 1; k < chunks; ++k) s += sums[k * kCoupleTerms + t];
        acc->sum[t] += s;
    } else if (t < kCoupleTerms) {
        unsigned long long s = 0ull;
        for (int k = 0; k < chunks; ++k) s += cnts[k * kCoupleTerms + t];
        acc->hits[t - kCoupleMax] += s;
    }
    if (t == 0) { acc->time += (double)dt; acc->substeps += 1ull; }
}

}  // namespace sph
