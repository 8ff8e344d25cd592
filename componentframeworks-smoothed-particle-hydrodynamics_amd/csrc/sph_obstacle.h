// sph_obstacle.h -- kinematic solid obstacles with fluid force and torque feedback (no reference counterpart).
//
// A body is a sphere, a box or a capsule whose pose and motion the caller prescribes.  After the SPH pass and the container, every
// non-ghost particle with finite coordinates meets bodies 0..K-1 in order; one strictly inside is projected onto the surface and, if it
// moves into the surface relative to the surface velocity, gets the body's wall response.  The per-particle arithmetic (obs_hit) and the
// pose advance (obs_advance) are __host__ __device__: sph_obstacles_apply_host / _advance_host run the same functions on the CPU.
// -ffp-contract=off: the only fused operations are the explicit fmaf() of dot3 (sph_device.h).
//
//   k_obstacles         sweeps over the output slots with a FIXED grid (min(kObsGrid, sweeps for n)): a world-AABB cull per body and
//                       wave, the hit, and per wave an xor butterfly of the six fp64 terms that lane 0 adds to its wave's LDS row; one
//                       partial row per block (its waves in order).  Reads pos, reads vel only near a body, writes back only what it changed.
//   k_obstacles_vol     k_obstacles for a set with a body bound to a volume (sph_volume.h): the binding and the volume slot are read at
//                       wave-uniform addresses like the bodies, the eight corner loads per evaluation are the only gathers.
//   k_obstacles_finish  one block: the partial rows summed in a fixed order (contiguous ranges, each ascending, then the ranges in order)
//                       into the accumulators, time += dt, substeps += 1, and every pose advanced by one substep.
//   k_obstacles_finish_dyn  k_obstacles_finish for a set with at least one dynamic body: the same sums, and body b
//                       stepped by thread b with this substep's own sums (obs_body_step) instead of only advanced.
// The bodies and the accumulators live in device memory, never in launch arguments, so a replayed graph sees every later
// sph_obstacles_set / _set_motion.  No float atomic is used: the sums depend on the slot order of the state (cell, id) only.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_kernels.h"
#include "sph_volume.h"   // built on it: a body may be bound to a volume (k_obstacles_vol)

namespace sph {

constexpr int kObsMax = 16;                  // SPH_MAX_OBSTACLES
constexpr int kObsTerms = 6;                 // Jx, Jy, Jz, Lx, Ly, Lz
constexpr int kObsRow = kObsMax * kObsTerms; // doubles per partial row
constexpr int kObsBlock = 512;               // threads per block of k_obstacles
constexpr int kObsFinishBlock = 1024;        // threads of k_obstacles_finish
constexpr int kObsUnroll = 2;                // slots per thread and sweep, their positions loaded together
constexpr int kObsSweep = kObsBlock * kObsUnroll;
constexpr int kObsGrid = 1024;               // blocks of k_obstacles at most: rows of the partial slab
constexpr int kObsWaves = kObsBlock / 64;
constexpr int kObsBatch = 16;                // k_obstacles_finish: loads in flight per thread
static_assert(kObsRow <= kObsFinishBlock, "k_obstacles_finish: at least one chunk of every term");
enum : int32_t { OBS_SPHERE = 0, OBS_BOX = 1, OBS_CAPSULE = 2 };

// Device record of one body (128 bytes).  M is the local -> world rotation, row major (world = M local), rebuilt from q; ext are the
// half extents of a conservative world AABB about c (a cull only: it never changes a result).
struct ObsRec {
    int32_t shape;
    float size[3];
    float c[3];
    float q[4];
    float M[9];
    float v[3];
    float w[3];
    float res, fr;
    float ext[3];
    float pad;
};
static_assert(sizeof(ObsRec) == 128, "ObsRec must be 128 bytes");

struct ObsAcc {
    double J[kObsRow];                       // (J, L) per body
    double time;                             // fp64 sum of dt
    unsigned long long substeps;
};

// q / |q|, |q| = sqrtf(fmaf(z, z, fmaf(y, y, fmaf(x, x, w * w)))), four IEEE divisions.
__host__ __device__ inline void obs_normalize(float (&q)[4]) {
    const float len = sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))));
    q[0] = q[0] / len; q[1] = q[1] / len; q[2] = q[2] / len; q[3] = q[3] / len;
}

// Rotation matrix of a unit quaternion (w, x, y, z), every operation rounded separately (identity for (1, 0, 0, 0)).
__host__ __device__ inline void obs_matrix(ObsRec& b) {
    const float w = b.q[0], x = b.q[1], y = b.q[2], z = b.q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    b.M[0] = 1.0f - 2.0f * (yy + zz); b.M[1] = 2.0f * (xy - wz);        b.M[2] = 2.0f * (xz + wy);
    b.M[3] = 2.0f * (xy + wz);        b.M[4] = 1.0f - 2.0f * (xx + zz); b.M[5] = 2.0f * (yz - wx);
    b.M[6] = 2.0f * (xz - wy);        b.M[7] = 2.0f * (yz + wx);        b.M[8] = 1.0f - 2.0f * (xx + yy);
}

// Conservative half extents of the world AABB about c (with a relative margin far above the rounding of the inside tests).
__host__ __device__ inline void obs_extent(ObsRec& b) {
    for (int i = 0; i < 3; ++i) {
        const float* m = b.M + 3 * i;
        float e;
        if (b.shape == OBS_SPHERE) e = b.size[0];
        else if (b.shape == OBS_BOX) e = fabsf(m[0]) * b.size[0] + fabsf(m[1]) * b.size[1] + fabsf(m[2]) * b.size[2];
        else e = fabsf(m[1]) * b.size[1] + b.size[0];
        b.ext[i] = e * 1.001f + 1e-6f;
    }
}

// One substep of the pose: c += dt V (a multiply, then an add); if omega != 0, q = normalize(q + (0.5f dt) (0, omega) (x) q) and M rebuilt.
__host__ __device__ inline void obs_advance(ObsRec& b, float dt) {
    for (int i = 0; i < 3; ++i) b.c[i] = b.c[i] + dt * b.v[i];
    const float ox = b.w[0], oy = b.w[1], oz = b.w[2];
    if (ox == 0.0f && oy == 0.0f && oz == 0.0f) return;             // a resting body's rotation keeps its bits
    const float w = b.q[0], x = b.q[1], y = b.q[2], z = b.q[3];
    const float pw = -((ox * x + oy * y) + oz * z);                  // Hamilton product (0, omega) (x) (w, x, y, z)
    const float px = (ox * w + oy * z) - oz * y;
    const float py = (oy * w + oz * x) - ox * z;
    const float pz = (oz * w + ox * y) - oy * x;
    const float hd = 0.5f * dt;
    b.q[0] = w + hd * pw; b.q[1] = x + hd * px; b.q[2] = y + hd * py; b.q[3] = z + hd * pz;
    obs_normalize(b.q);
    obs_matrix(b);
    obs_extent(b);
}

// One body against one particle.  Returns false (nothing changed) unless the particle is strictly inside; then p is
// projected onto the surface, v gets the wall response if u_n < 0, and t receives (J, L) in fp64 (zeros when u_n >= 0).
// VOL: a box bound to a volume (vol != nullptr) is box, lattice extent and {phi < 0} intersected; the lattice gives
// the projected point and the normal (vol_project), or leaves both to the box where its gradient vanishes.
template <bool VOL>
__host__ __device__ inline bool obs_hit_t(const ObsRec& b, const VolRec* vol, float mass, float& px, float& py, float& pz, float& vx, float& vy,
                                          float& vz, double (&t)[kObsTerms]) {
    const float dx = px - b.c[0], dy = py - b.c[1], dz = pz - b.c[2];
    const float* M = b.M;
    float nx, ny, nz, qx, qy, qz;                                    // world normal, projected world point
    if (b.shape == OBS_SPHERE) {
        const float R = b.size[0];
        const float r2 = dot3(dx, dy, dz, dx, dy, dz);
        if (!(r2 < R * R)) return false;
        const float len = sqrtf(r2);
        if (len == 0.0f) { nx = M[1]; ny = M[4]; nz = M[7]; }       // the exact centre: local +y
        else { nx = dx / len; ny = dy / len; nz = dz / len; }
        qx = b.c[0] + R * nx; qy = b.c[1] + R * ny; qz = b.c[2] + R * nz;
    } else {
        const float lx = dot3(dx, dy, dz, M[0], M[3], M[6]);      // l = M^T (p - c)
        const float ly = dot3(dx, dy, dz, M[1], M[4], M[7]);
        const float lz = dot3(dx, dy, dz, M[2], M[5], M[8]);
        float ox, oy, oz, mx, my, mz;                                // local projected point, local normal
        if (b.shape == OBS_BOX) {
            const float hx = b.size[0], hy = b.size[1], hz = b.size[2];
            if (!(fabsf(lx) < hx && fabsf(ly) < hy && fabsf(lz) < hz)) return false;
            const float ax = hx - fabsf(lx), ay = hy - fabsf(ly), az = hz - fabsf(lz);
            ox = lx; oy = ly; oz = lz; mx = 0.0f; my = 0.0f; mz = 0.0f;
            int how = 2;                                             // 0: no hit, 1: the lattice projected, 2: the nearest face of the box
            if constexpr (VOL) {
                if (vol) how = vol_project(*vol, lx, ly, lz, ox, oy, oz, mx, my, mz);
            }
            if (how == 0) return false;
            if (how == 1) {}
            else if (ax <= ay && ax <= az) { const float s = lx >= 0.0f ? 1.0f : -1.0f; ox = s * hx; mx = s; }   // ties: x, then y, then z
            else if (ay <= az) { const float s = ly >= 0.0f ? 1.0f : -1.0f; oy = s * hy; my = s; }
            else { const float s = lz >= 0.0f ? 1.0f : -1.0f; oz = s * hz; mz = s; }
        } else {
            const float r = b.size[0], L = b.size[1];
            const float sy = fminf(fmaxf(ly, -L), L);
            const float ex = lx, ey = ly - sy, ez = lz;
            const float e2 = dot3(ex, ey, ez, ex, ey, ez);
            if (!(e2 < r * r)) return false;
            const float len = sqrtf(e2);
            if (len == 0.0f) { mx = 1.0f; my = 0.0f; mz = 0.0f; }   // on the core segment: local +x
            else { mx = ex / len; my = ey / len; mz = ez / len; }
            ox = r * mx; oy = sy + r * my; oz = r * mz;
        }
        nx = dot3(M[0], M[1], M[2], mx, my, mz);
        ny = dot3(M[3], M[4], M[5], mx, my, mz);
        nz = dot3(M[6], M[7], M[8], mx, my, mz);
        qx = b.c[0] + dot3(M[0], M[1], M[2], ox, oy, oz);
        qy = b.c[1] + dot3(M[3], M[4], M[5], ox, oy, oz);
        qz = b.c[2] + dot3(M[6], M[7], M[8], ox, oy, oz);
    }
    const float rx = qx - b.c[0], ry = qy - b.c[1], rz = qz - b.c[2];
    const float sx = b.v[0] + (b.w[1] * rz - b.w[2] * ry);           // surface velocity V + omega x r
    const float sy = b.v[1] + (b.w[2] * rx - b.w[0] * rz);
    const float sz = b.v[2] + (b.w[0] * ry - b.w[1] * rx);
    const float ux = vx - sx, uy = vy - sy, uz = vz - sz;
    const float un = dot3(ux, uy, uz, nx, ny, nz);
    px = qx; py = qy; pz = qz;
    for (int i = 0; i < kObsTerms; ++i) t[i] = 0.0;
    if (un < 0.0f) {
        const float a = -b.res * un, omf = 1.0f - b.fr;
        const float tx = ux - un * nx, ty = uy - un * ny, tz = uz - un * nz;
        const float wx = (sx + a * nx) + omf * tx, wy = (sy + a * ny) + omf * ty, wz = (sz + a * nz) + omf * tz;
        const double m = (double)mass;
        t[0] = m * ((double)vx - (double)wx);
        t[1] = m * ((double)vy - (double)wy);
        t[2] = m * ((double)vz - (double)wz);
        const double Rx = (double)rx, Ry = (double)ry, Rz = (double)rz;
        t[3] = Ry * t[2] - Rz * t[1];
        t[4] = Rz * t[0] - Rx * t[2];
        t[5] = Rx * t[1] - Ry * t[0];
        vx = wx; vy = wy; vz = wz;
    }
    return true;
}
__host__ __device__ inline bool obs_hit(const ObsRec& b, float mass, float& px, float& py, float& pz, float& vx, float& vy, float& vz,
                                        double (&t)[kObsTerms]) {
    return obs_hit_t<false>(b, nullptr, mass, px, py, pz, vx, vy, vz, t);
}

// One slot against bodies 0..K-1 in order (slot s of the output state, its position already loaded): the wave's terms of every body that
// some lane of the wave is near go through an xor butterfly, and lane 0 adds them to the wave's LDS row.
__device__ __forceinline__ bool obs_near(const ObsRec& B, float4 P) {
    return fabsf(P.x - B.c[0]) <= B.ext[0] && fabsf(P.y - B.c[1]) <= B.ext[1] && fabsf(P.z - B.c[2]) <= B.ext[2];
}
// The bodies are read from global memory at wave-uniform addresses (scalar loads: the cull compares against SGPRs).
// VOL: the binding of body b and the slot it names are read from the table at wave-uniform addresses as well.
template <bool VOL>
__device__ __forceinline__ void obs_slot(const ObsRec* __restrict__ bodies, const VolTable* __restrict__ tab, int K, float mass,
                                         float4* __restrict__ pos, float4* __restrict__ vel, int s, float4 P, bool cand, double* row, int lane) {
    float4 V = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool haveV = false, changed = false;
    for (int b = 0; b < K; ++b) {
        const ObsRec& B = bodies[b];
        const bool near = cand && obs_near(B, P);
        if (__ballot(near) == 0ull) continue;                         // (wave-uniform)
        double t[kObsTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (near) {
            if (!haveV) { V = vel[s]; haveV = true; }
            const VolRec* vol = nullptr;
            if constexpr (VOL) {
                const int id = tab->bind[b];
                if (id >= 0) vol = &tab->vol[id];
            }
            changed |= obs_hit_t<VOL>(B, vol, mass, P.x, P.y, P.z, V.x, V.y, V.z, t);
        }
#pragma unroll
        for (int c = 0; c < kObsTerms; ++c)
            for (int o = 32; o >= 1; o >>= 1) t[c] += __shfl_xor(t[c], o, 64);   // (open-coded: wave_sum per term reorders the independent chains; profiles/r20_header_refactor_ab.json)
        if (lane == 0)
            for (int c = 0; c < kObsTerms; ++c) row[b * kObsTerms + c] += t[c];
    }
    if (changed) { pos[s] = P; vel[s] = V; }
}

// Sweeps of kObsSweep slots: slot base + j kObsBlock + thread for j = 0 .. kObsUnroll - 1.  The kObsUnroll positions are loaded together,
// then the slots are processed in j order (a velocity is loaded at the first body the slot is near).  One partial row per block: its
// waves' rows summed in wave order.
__global__ __launch_bounds__(kObsBlock) void k_obstacles(const ObsRec* __restrict__ bodies, int K, float mass, float4* __restrict__ pos,
                                                         float4* __restrict__ vel, int n, double* __restrict__ part) {
    __shared__ double sacc[kObsWaves][kObsRow];
    {
        double* z = &sacc[0][0];
        for (int i = threadIdx.x; i < kObsWaves * kObsRow; i += kObsBlock) z[i] = 0.0;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int base = blockIdx.x * kObsSweep; base < n; base += gridDim.x * kObsSweep) {     // (block-uniform)
        float4 P[kObsUnroll];
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            P[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < n) P[j] = pos[s];
        }
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            const bool cand = s < n && !(fbits(P[j].w) & (F_GHOSTNZ | F_HALO)) && float_finite(P[j].x) && float_finite(P[j].y) && float_finite(P[j].z);
            obs_slot<false>(bodies, nullptr, K, mass, pos, vel, s, P[j], cand, sacc[wave], lane);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * kObsTerms; i += kObsBlock) {
        double r = sacc[0][i];
        for (int w = 1; w < kObsWaves; ++w) r += sacc[w][i];
        part[(size_t)blockIdx.x * kObsRow + i] = r;
    }
}
// One block.  The rows are cut into chunks = min(kObsFinishBlock / (6 K), rows) contiguous ranges of ceil(rows / chunks); thread
// (chunk, term) sums its range in ascending row order (loads issued kObsBatch at a time), then thread `term` sums the chunk sums in chunk
// order and adds the result to the accumulator.  Then the poses advance.
__global__ __launch_bounds__(kObsFinishBlock) void k_obstacles_finish(ObsRec* __restrict__ bodies, int K, float dt, const double* __restrict__ part,
                                                                int rows, ObsAcc* __restrict__ acc) {
    __shared__ double sums[kObsFinishBlock];
    const int terms = K * kObsTerms, chunks = max(1, min(kObsFinishBlock / max(terms, 1), rows));
    const int t = threadIdx.x, c = t % max(terms, 1), ch = t / max(terms, 1);
    if (ch < chunks && c < terms) {
        const int per = (rows + chunks - 1) / chunks;
        const int r1 = min(rows, (ch + 1) * per);
        int r = ch * per;
        double s = 0.0;
        for (; r + kObsBatch <= r1; r += kObsBatch) {
            double v[kObsBatch];
#pragma unroll
            for (int j = 0; j < kObsBatch; ++j) v[j] = part[(size_t)(r + j) * kObsRow + c];
#pragma unroll
            for (int j = 0; j < kObsBatch; ++j) s += v[j];
        }
        for (; r < r1; ++r) s += part[(size_t)r * kObsRow + c];
        sums[ch * terms + c] = s;
    }
    __syncthreads();
    if (t < terms) {
        double s = sums[t];
        for (int k = 1; k < chunks; ++k) s += sums[k * terms + t];
        acc->J[t] += s;
    }
    if (t == 0) { acc->time += (double)dt; acc->substeps += 1ull; }
    if (t < K) {
        ObsRec B = bodies[t];
        obs_advance(B, dt);
        bodies[t] = B;
    }
}

// The same pass for a set with at least one body bound to a volume (launched only then: DESIGN.md section 3f).  The body is written out a
// second time on purpose: with both kernels calling one shared function template, k_obstacles no longer compiled to the instructions it
// had before volumes existed (another register allocation), and the primitive path must not pay for this one.  It is defined after
// k_obstacles_finish so that the finish stays next to k_obstacles in the code object: with this kernel between them the one-block finish,
// the same instructions, ran 0.9 us slower in a kernel trace (12.9 against 11.9 us) and the pass without volumes 1-2 us slower than before.
__global__ __launch_bounds__(kObsBlock) void k_obstacles_vol(const ObsRec* __restrict__ bodies, const VolTable* __restrict__ tab, int K, float mass,
                                                             float4* __restrict__ pos, float4* __restrict__ vel, int n, double* __restrict__ part) {
    __shared__ double sacc[kObsWaves][kObsRow];
    {
        double* z = &sacc[0][0];
        for (int i = threadIdx.x; i < kObsWaves * kObsRow; i += kObsBlock) z[i] = 0.0;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int base = blockIdx.x * kObsSweep; base < n; base += gridDim.x * kObsSweep) {     // (block-uniform)
        float4 P[kObsUnroll];
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            P[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < n) P[j] = pos[s];
        }
#pragma unroll
        for (int j = 0; j < kObsUnroll; ++j) {
            const int s = base + j * kObsBlock + threadIdx.x;
            const bool cand = s < n && !(fbits(P[j].w) & (F_GHOSTNZ | F_HALO)) && float_finite(P[j].x) && float_finite(P[j].y) && float_finite(P[j].z);
            obs_slot<true>(bodies, tab, K, mass, pos, vel, s, P[j], cand, sacc[wave], lane);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * kObsTerms; i += kObsBlock) {
        double r = sacc[0][i];
        for (int w = 1; w < kObsWaves; ++w) r += sacc[w][i];
        part[(size_t)blockIdx.x * kObsRow + i] = r;
    }
}

// ---- dynamic bodies ---------------------------------------------------------
// A body with a dynamics record moves under the substep's own sums (J, L): k_obstacles_finish_dyn is launched instead of
// k_obstacles_finish while at least one body has a record (k_obstacles_finish itself stays what it is for kinematic sets).  The body step
// (obs_body_step) is __host__ __device__ and is what sph_obstacles_step_host runs.  fp32, every operation rounded on its own except
// dot3; the J and L terms are fp64.
struct ObsDyn {                              // 128 bytes, one per body, beside ObsRec
    int32_t active;                          // 0: kinematic
    float mass;
    float I[6], Iinv[6];                     // xx, yy, zz, xy, xz, yz about the centre of mass, body frame; Iinv inverted in fp64 on set
    float com[3];
    float gscale;
    float force[3], torque[3];
    float ldamp, adamp;
    uint32_t flags;                          // bit 0: confined by the container
    float pad[5];
};
static_assert(sizeof(ObsDyn) == 128, "ObsDyn must be 128 bytes");
enum : uint32_t { OBS_DYN_CONFINED = 1u };

// What the body step needs of the scene: gravity, the container's oriented box (axis j in world coordinates is A[3 j .. 3 j + 2]) and
// the wall restitution.
struct ObsWorld {
    float g[3];
    float bc[3];
    float A[9];
    float half[3];
    float rest;
};

// M (S (M^T x)) for a symmetric S = (xx, yy, zz, xy, xz, yz) in the body frame: three rows of dot3 each.
__host__ __device__ inline void obs_sym_world(const float* M, const float* S, const float (&x)[3], float (&out)[3]) {
    const float l0 = dot3(x[0], x[1], x[2], M[0], M[3], M[6]);
    const float l1 = dot3(x[0], x[1], x[2], M[1], M[4], M[7]);
    const float l2 = dot3(x[0], x[1], x[2], M[2], M[5], M[8]);
    const float s0 = dot3(S[0], S[3], S[4], l0, l1, l2);
    const float s1 = dot3(S[3], S[1], S[5], l0, l1, l2);
    const float s2 = dot3(S[4], S[5], S[2], l0, l1, l2);
    out[0] = dot3(M[0], M[1], M[2], s0, s1, s2);
    out[1] = dot3(M[3], M[4], M[5], s0, s1, s2);
    out[2] = dot3(M[6], M[7], M[8], s0, s1, s2);
}
__host__ __device__ inline void obs_cross(const float (&a)[3], const float (&b)[3], float (&out)[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// Support points of a body in its own frame (fixed order) and their radius.
__host__ __device__ inline int obs_support(const ObsRec& B, float (&lp)[8][3], float& rad) {
    if (B.shape == OBS_SPHERE) { lp[0][0] = 0.0f; lp[0][1] = 0.0f; lp[0][2] = 0.0f; rad = B.size[0]; return 1; }
    if (B.shape == OBS_CAPSULE) {
        lp[0][0] = 0.0f; lp[0][1] = -B.size[1]; lp[0][2] = 0.0f;
        lp[1][0] = 0.0f; lp[1][1] = B.size[1]; lp[1][2] = 0.0f;
        rad = B.size[0];
        return 2;
    }
    for (int i = 0; i < 8; ++i) {            // corner i: bit 0 -> +x, bit 1 -> +y, bit 2 -> +z
        lp[i][0] = (i & 1) ? B.size[0] : -B.size[0];
        lp[i][1] = (i & 2) ? B.size[1] : -B.size[1];
        lp[i][2] = (i & 4) ? B.size[2] : -B.size[2];
    }
    rad = 0.0f;
    return 8;
}

// One substep of a dynamic body: S = (J, L) of this substep about the geometric centre.
__host__ __device__ inline void obs_body_step(ObsRec& B, const ObsDyn& D, const double* S, const ObsWorld& W, float dt) {
    const float* M = B.M;
    // 1. to the centre of mass
    float o[3];
    o[0] = dot3(M[0], M[1], M[2], D.com[0], D.com[1], D.com[2]);
    o[1] = dot3(M[3], M[4], M[5], D.com[0], D.com[1], D.com[2]);
    o[2] = dot3(M[6], M[7], M[8], D.com[0], D.com[1], D.com[2]);
    const double O0 = (double)o[0], O1 = (double)o[1], O2 = (double)o[2];
    float Lg[3];
    Lg[0] = (float)(S[3] - (O1 * S[2] - O2 * S[1]));
    Lg[1] = (float)(S[4] - (O2 * S[0] - O0 * S[2]));
    Lg[2] = (float)(S[5] - (O0 * S[1] - O1 * S[0]));
    float w[3] = {B.w[0], B.w[1], B.w[2]};
    float x[3], Vg[3];
    obs_cross(w, o, x);
    for (int a = 0; a < 3; ++a) Vg[a] = B.v[a] + x[a];
    // 2. linear velocity
    for (int a = 0; a < 3; ++a) {
        const float acc = D.gscale * W.g[a] + D.force[a] / D.mass;
        Vg[a] = (Vg[a] + (float)(S[a] / (double)D.mass)) + dt * acc;
    }
    // 3. angular velocity
    {
        float Iw[3], gy[3], rhs[3], dw[3];
        obs_sym_world(M, D.I, w, Iw);
        obs_cross(w, Iw, gy);
        for (int a = 0; a < 3; ++a) rhs[a] = Lg[a] + dt * (D.torque[a] - gy[a]);
        obs_sym_world(M, D.Iinv, rhs, dw);
        for (int a = 0; a < 3; ++a) w[a] = w[a] + dw[a];
    }
    // 4. damping
    {
        const float fl = fmaxf(0.0f, 1.0f - D.ldamp * dt), fa = fmaxf(0.0f, 1.0f - D.adamp * dt);
        for (int a = 0; a < 3; ++a) { Vg[a] = Vg[a] * fl; w[a] = w[a] * fa; }
    }
    // 5. container contact at the entry pose: faces -x, +x, -y, +y, -z, +z, support points in order
    if (D.flags & OBS_DYN_CONFINED) {
        float lp[8][3], rad;
        const int np = obs_support(B, lp, rad);
        float pen[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const float im = 1.0f / D.mass, ope = 1.0f + W.rest;
        for (int f = 0; f < 6; ++f) {
            const int j = f >> 1;
            const float sg = (f & 1) ? -1.0f : 1.0f;                 // inward normal: +axis at the low face, -axis at the high face
            const float n[3] = {sg * W.A[3 * j], sg * W.A[3 * j + 1], sg * W.A[3 * j + 2]};
            for (int p = 0; p < np; ++p) {
                float s[3], r[3], d[3];
                s[0] = dot3(M[0], M[1], M[2], lp[p][0], lp[p][1], lp[p][2]);
                s[1] = dot3(M[3], M[4], M[5], lp[p][0], lp[p][1], lp[p][2]);
                s[2] = dot3(M[6], M[7], M[8], lp[p][0], lp[p][1], lp[p][2]);
                for (int a = 0; a < 3; ++a) { r[a] = s[a] - o[a]; d[a] = (B.c[a] + s[a]) - W.bc[a]; }
                const float dist = W.half[j] + dot3(d[0], d[1], d[2], n[0], n[1], n[2]);   // distance of the point from the face, inward
                const float depth = rad - dist;
                if (!(depth >= 0.0f)) continue;                       // (touching counts: a body at rest on a face stays in contact)
                if (depth > pen[f]) pen[f] = depth;
                float wr[3], rn[3], k3[3], kr[3];
                obs_cross(w, r, wr);
                const float vn = dot3(Vg[0] + wr[0], Vg[1] + wr[1], Vg[2] + wr[2], n[0], n[1], n[2]);
                if (!(vn < 0.0f)) continue;
                obs_cross(r, n, rn);
                obs_sym_world(M, D.Iinv, rn, k3);
                obs_cross(k3, r, kr);
                const float den = im + dot3(n[0], n[1], n[2], kr[0], kr[1], kr[2]);
                const float jn = (-ope * vn) / den;
                const float jm = jn * im;
                for (int a = 0; a < 3; ++a) { Vg[a] = Vg[a] + jm * n[a]; w[a] = w[a] + jn * k3[a]; }
            }
        }
        for (int f = 0; f < 6; ++f) {
            if (!(pen[f] > 0.0f)) continue;
            const int j = f >> 1;
            const float sg = (f & 1) ? -1.0f : 1.0f;
            for (int a = 0; a < 3; ++a) B.c[a] = B.c[a] + pen[f] * (sg * W.A[3 * j + a]);
        }
    }
    // 6. back to the geometric centre, 7. the pose advance with the new velocities
    obs_cross(w, o, x);
    for (int a = 0; a < 3; ++a) { B.v[a] = Vg[a] - x[a]; B.w[a] = w[a]; }
    obs_advance(B, dt);
}

// k_obstacles_finish for a set with at least one dynamic body (launched only then).  The sums are formed exactly as k_obstacles_finish
// forms them; this substep's sums also go to LDS, and thread b steps body b with them (obs_body_step) or, for a kinematic body, advances it.
__global__ __launch_bounds__(kObsFinishBlock) void k_obstacles_finish_dyn(ObsRec* __restrict__ bodies, const ObsDyn* __restrict__ dyn, ObsWorld W, int K,
                                                                          float dt, const double* __restrict__ part, int rows, ObsAcc* __restrict__ acc) {
    __shared__ double sums[kObsFinishBlock];
    __shared__ double sub[kObsRow];
    const int terms = K * kObsTerms, chunks = max(1, min(kObsFinishBlock / max(terms, 1), rows));
    const int t = threadIdx.x, c = t % max(terms, 1), ch = t / max(terms, 1);
    if (ch < chunks && c < terms) {
        const int per = (rows + chunks - 1) / chunks;
        const int r1 = min(rows, (ch + 1) * per);
        int r = ch * per;
        double s = 0.0;
        for (; r + kObsBatch <= r1; r += kObsBatch) {
            double v[kObsBatch];
#pragma unroll
            for (int j = 0; j < kObsBatch; ++j) v[j] = part[(size_t)(r + j) * kObsRow + c];
#pragma unroll
            for (int j = 0; j < kObsBatch; ++j) s += v[j];
        }
        for (; r < r1; ++r) s += part[(size_t)r * kObsRow + c];
        sums[ch * terms + c] = s;
    }
    __syncthreads();
    if (t < terms) {
        double s = sums[t];
        for (int k = 1; k < chunks; ++k) s += sums[k * terms + t];
        sub[t] = s;
        acc->J[t] += s;
    }
    if (t == 0) { acc->time += (double)dt; acc->substeps += 1ull; }
    __syncthreads();
    if (t < K) {
        ObsRec B = bodies[t];
        const ObsDyn D = dyn[t];
        if (D.active) obs_body_step(B, D, sub + t * kObsTerms, W, dt);
        else obs_advance(B, dt);
        bodies[t] = B;
    }
}

}  // namespace sph
