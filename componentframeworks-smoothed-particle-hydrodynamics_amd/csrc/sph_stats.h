// sph_stats.h -- totals, extrema, occupancy and histograms of the particle state (no reference counterpart).
//
// Input is the grid of the current state: the sorted copy k_rank writes (pv: pos, 1/rho | vel, P; own: cell, foam, flags, id), the
// exact density gathered through order[] (k_rank<true, true> fills it for every slot) and cellStart.
//
//   k_stats_tiles   a block per tile of kStatTile = 2048 consecutive slots (at most kStatGrid blocks, each striding over the tiles): the
//                   15 fp64 sums of the tile by the FIXED halving tree x[i] += x[i + s], s = 1024 .. 1 (thread t holds slots t + 256 j,
//                   so s = 1024, 512, 256 stay inside the thread, s = 128, 64 cross the waves through LDS, s = 32 .. 1 are an xor
//                   butterfly in wave 0), the 12 (value, id) extrema, the counts, and the requested histograms in LDS; 15 sums per
//                   tile, one partial record and one histogram row per block
//   k_stats_cells   occupancy of the cells from cellStart; one partial row per block
//   k_stats_finish  17 blocks: one per sum for the halving tree over the tile sums padded to a power of two (in LDS up to
//                   kStatTreeLds tiles, in place in global memory beyond), one for the blocks' partial records, one for the cells' rows
//   k_stats_hist    sums the blocks' histogram rows into 64-bit counters
//
// Every cross-block combination is store-and-sum over a scratch slab: no global atomics, so nothing depends on arrival order, and the
// order of the fp64 additions is the one DESIGN.md writes down whatever the launch shape.
#pragma once
#include "sph_kernels.h"

namespace sph {

constexpr int kStatTile = 2048;
constexpr int kStatPer = kStatTile / kBlock;            // slots per thread
constexpr int kStatSums = 15;
constexpr int kStatExt = 12;
constexpr int kStatCnt = 7;
constexpr int kStatMaxSpecs = 4, kStatMaxBins = 1024;
constexpr int kStatHistWords = kStatMaxSpecs * (kStatMaxBins + 2);
static_assert(66 % 22 == 0, "k_stats_finish reads the cells' slab 22 columns at a time");
constexpr int kStatCellCols = 66;                       // occupancy[65] + the packed (count, ~index) maximum
constexpr int kStatCellBlocks = 256;
constexpr int kStatGrid = 1024;                        // blocks of k_stats_tiles: rows of the partial slabs
constexpr int kStatTreeLds = 4096;                      // tile sums one block reduces in LDS (32 KiB): 8 M particles
static_assert(kStatCellBlocks <= kBlock, "k_stats_finish reads one row of the cells' slab per thread");
static_assert(kStatPer == 8 && kBlock == 256, "the in-thread part of the tree is written out for 8 slots per thread");

// sums: 0-2 pos, 3-5 vel, 6 v2, 7 rho, 8 rho^2, 9 P, 10 foam, 11 1/rho, 12-14 (pos - c) x vel
// extrema: 0-2 min pos, 3-5 max pos, 6 min rho, 7 max rho, 8 min P, 9 max P, 10 max foam, 11 max speed2
// counts: 0 fluid, 1 active ghosts, 2 inactive ghosts, 3 other, 4 non-finite, 5 counted, 6 escaped
__host__ __device__ constexpr bool stat_is_min(int k) { return k < 3 || k == 6 || k == 8; }

struct StatK {
    float gminx, gminy, gminz, cellSize;
    float gx, gy, gz;                    // grid dimensions as floats (<= 1024: exact)
    double cx, cy, cz;                   // param_boxCenter
    int n, nTiles, tilesPow2, numCells;
    int nBlocks;                         // grid of k_stats_tiles
    int nSpecs;
    uint32_t histWords;                  // sum of bins + 2 over the specs
    int field[kStatMaxSpecs];
    uint32_t bins[kStatMaxSpecs], off[kStatMaxSpecs];
    float lo[kStatMaxSpecs], hi[kStatMaxSpecs], scale[kStatMaxSpecs];     // scale = (float)bins / (hi - lo), divided on the host in fp32
};

// Partial record of a block of k_stats_tiles, stored word by word across the blocks (word w of block b at part[w * kStatGrid + b], so
// k_stats_finish reads it coalesced): 12 extreme values (float bits), their 12 ids, 7 counts, lowest non-finite id, lowest escaped id.
constexpr int kStatPartWords = 2 * kStatExt + kStatCnt + 2;

// (value, id) pairs: the lower value (min) or higher value (max) wins, of two that compare equal the lower id.  No NaN reaches this.
__device__ __forceinline__ void stat_take(bool isMin, float& v, uint32_t& id, float v2, uint32_t id2) {
    const bool better = isMin ? (v2 < v) : (v < v2);
    const bool worse = isMin ? (v < v2) : (v2 < v);
    if (better || (!worse && id2 < id)) { v = v2; id = id2; }
}
__device__ __forceinline__ void stat_wave_ext(float (&ev)[kStatExt], uint32_t (&eid)[kStatExt]) {
#pragma unroll
    for (int k = 0; k < kStatExt; ++k)
        for (int s = 32; s >= 1; s >>= 1) {
            const float v2 = __shfl_xor(ev[k], s, 64);
            const uint32_t id2 = (uint32_t)__shfl_xor((int)eid[k], s, 64);
            stat_take(stat_is_min(k), ev[k], eid[k], v2, id2);
        }
}

__device__ __forceinline__ uint32_t stat_bin(float v, float lo, float hi, float scale, uint32_t bins) {
    if (v < lo) return 0u;
    if (v >= hi) return bins + 1u;
    const float f = floorf((v - lo) * scale);                          // >= 0 and finite here
    return 1u + (f < (float)(bins - 1u) ? (uint32_t)(int)f : bins - 1u);
}

// One slot: its 15 terms (+0.0 outside the counted set and beyond n), the extrema, the wave's counts, the histograms.  rho: the exact
// density; it and the slot's sorted records (a: pos, b: vel + P, o: own) are loaded by the caller, zeros beyond n.
__device__ __forceinline__ void stat_slot(const StatK& k, bool in, float4 a, float4 b, float4 o, float rho, double (&t)[kStatSums],
                                          float (&ev)[kStatExt], uint32_t (&eid)[kStatExt], uint32_t (&cnt)[kStatCnt], uint32_t (&first)[2],
                                          uint32_t* smHist) {
#pragma unroll
    for (int i = 0; i < kStatSums; ++i) t[i] = 0.0;
    const uint32_t flags = fbits(o.z), id = fbits(o.w);
    const float foam = o.y, prs = b.w;
    const bool fluid = in && !(flags & F_GHOSTNZ);
    const bool g1 = in && (flags & F_GHOST1);
    const bool finite = float_finite(a.x) && float_finite(a.y) && float_finite(a.z) && float_finite(b.x) && float_finite(b.y) && float_finite(b.z) &&
                        float_finite(rho) && float_finite(prs) && float_finite(foam);
    const bool counted = fluid && finite;
    const bool bad = fluid && !finite;
    const float qx = floorf((a.x - k.gminx) / k.cellSize), qy = floorf((a.y - k.gminy) / k.cellSize), qz = floorf((a.z - k.gminz) / k.cellSize);
    const bool escaped = counted && (qx < 0.0f || qx >= k.gx || qy < 0.0f || qy >= k.gy || qz < 0.0f || qz >= k.gz);
    cnt[0] += (uint32_t)__popcll(__ballot(fluid));
    cnt[1] += (uint32_t)__popcll(__ballot(g1 && !(flags & F_INACTIVE)));
    cnt[2] += (uint32_t)__popcll(__ballot(g1 && (flags & F_INACTIVE)));
    cnt[3] += (uint32_t)__popcll(__ballot(in && (flags & F_GHOSTNZ) && !(flags & F_GHOST1)));
    cnt[4] += (uint32_t)__popcll(__ballot(bad));
    cnt[5] += (uint32_t)__popcll(__ballot(counted));
    cnt[6] += (uint32_t)__popcll(__ballot(escaped));
    if (bad) first[0] = min(first[0], id);
    if (escaped) first[1] = min(first[1], id);
    if (!counted) return;
    const float speed2 = (b.x * b.x + b.y * b.y) + b.z * b.z;
    const float val[kStatExt] = {a.x, a.y, a.z, a.x, a.y, a.z, rho, rho, prs, prs, foam, speed2};
#pragma unroll
    for (int e = 0; e < kStatExt; ++e) stat_take(stat_is_min(e), ev[e], eid[e], val[e], id);
    const double x = (double)a.x, y = (double)a.y, z = (double)a.z, vx = (double)b.x, vy = (double)b.y, vz = (double)b.z, r = (double)rho;
    t[0] = x; t[1] = y; t[2] = z;
    t[3] = vx; t[4] = vy; t[5] = vz;
    t[6] = (vx * vx + vy * vy) + vz * vz;
    t[7] = r;
    t[8] = r * r;
    t[9] = (double)prs;
    t[10] = (double)foam;
    t[11] = rho > 0.0f ? 1.0 / r : 0.0;
    const double dx = x - k.cx, dy = y - k.cy, dz = z - k.cz;
    t[12] = dy * vz - dz * vy;
    t[13] = dz * vx - dx * vz;
    t[14] = dx * vy - dy * vx;
    for (int s = 0; s < k.nSpecs; ++s) {
        const int f = k.field[s];
        const float v = f == 0 ? rho : f == 1 ? prs : f == 2 ? sqrtf(speed2) : f == 3 ? a.x : f == 4 ? a.y : f == 5 ? a.z : foam;
        atomicAdd(&smHist[k.off[s] + stat_bin(v, k.lo[s], k.hi[s], k.scale[s], k.bins[s])], 1u);
    }
}

__global__ __launch_bounds__(kBlock) void k_stats_tiles(StatK k, const float4* __restrict__ pv, const float4* __restrict__ own,
                                                        const uint32_t* __restrict__ order, const float2* __restrict__ rp,
                                                        double* __restrict__ tileSums, uint32_t* __restrict__ part,
                                                        uint32_t* __restrict__ tileHist) {
    __shared__ double smSum[kStatSums * (kBlock / 2)];
    __shared__ uint32_t smHist[kStatHistWords];
    __shared__ float smEv[kBlock / 64][kStatExt];
    __shared__ uint32_t smEid[kBlock / 64][kStatExt];
    __shared__ uint32_t smCnt[kStatCnt], smFirst[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < k.histWords; i += kBlock) smHist[i] = 0u;
    if (tid < kStatCnt) smCnt[tid] = 0u;
    if (tid < 2) smFirst[tid] = 0xFFFFFFFFu;
    __syncthreads();

    float ev[kStatExt];
    uint32_t eid[kStatExt], cnt[kStatCnt], first[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int e = 0; e < kStatExt; ++e) { ev[e] = stat_is_min(e) ? INFINITY : -INFINITY; eid[e] = 0xFFFFFFFFu; }
#pragma unroll
    for (int c = 0; c < kStatCnt; ++c) cnt[c] = 0u;

    for (int tile = blockIdx.x; tile < k.nTiles; tile += gridDim.x) {
    // s = 1024, 512, 256 of the tree inside the thread: ((x0 + x4) + (x2 + x6)) + ((x1 + x5) + (x3 + x7)), x_j = slot base + tid + 256 j
    const int base = tile * kStatTile + tid;
    double acc[kStatSums];
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        // the gather of this half's exact densities first, all four in flight (j = half + 2 q + 4 side); order[] is nearly monotone, the
        // state keeps the previous substep's order
        uint32_t src[4];
        float rho[4];
        float4 A[4], B[4], O[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int slot = base + kBlock * (half + 2 * u);
            const bool in = slot < k.n;
            src[u] = in ? order[slot] : 0u;
            A[u] = in ? pv[2 * (size_t)slot] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            B[u] = in ? pv[2 * (size_t)slot + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            O[u] = in ? own[slot] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) rho[u] = base + kBlock * (half + 2 * u) < k.n ? rp[src[u]].x : 0.0f;
        double grp[kStatSums];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ja = half + 2 * q;
            double ta[kStatSums], tb[kStatSums];
            stat_slot(k, base + kBlock * ja < k.n, A[q], B[q], O[q], rho[q], ta, ev, eid, cnt, first, smHist);
            stat_slot(k, base + kBlock * (ja + 4) < k.n, A[q + 2], B[q + 2], O[q + 2], rho[q + 2], tb, ev, eid, cnt, first, smHist);
#pragma unroll
            for (int i = 0; i < kStatSums; ++i) {
                const double y = ta[i] + tb[i];
                grp[i] = q == 0 ? y : grp[i] + y;
            }
        }
#pragma unroll
        for (int i = 0; i < kStatSums; ++i) acc[i] = half == 0 ? grp[i] : acc[i] + grp[i];
    }
    // s = 128, 64 across the waves
    if (tid >= 128) {
#pragma unroll
        for (int i = 0; i < kStatSums; ++i) smSum[i * 128 + (tid - 128)] = acc[i];
    }
    __syncthreads();
    if (tid < 128) {
#pragma unroll
        for (int i = 0; i < kStatSums; ++i) acc[i] = acc[i] + smSum[i * 128 + tid];
    }
    __syncthreads();
    if (tid >= 64 && tid < 128) {
#pragma unroll
        for (int i = 0; i < kStatSums; ++i) smSum[i * 128 + (tid - 64)] = acc[i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < kStatSums; ++i) {
            double v = acc[i] + smSum[i * 128 + tid];
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);            // lane 0: x[0] += x[s], the tree's last six steps
            if (lane == 0) tileSums[(size_t)i * k.tilesPow2 + tile] = v;
        }
    }
    __syncthreads();                                                                    // (smSum is written again by the next tile)
    }
    // extrema, counts, first ids: any tree gives the same bits
    stat_wave_ext(ev, eid);
    for (int s = 32; s >= 1; s >>= 1) {                                                 // (open-coded, like the loops below: the calls of sph_wave.h
        first[0] = min(first[0], (uint32_t)__shfl_xor((int)first[0], s, 64));           // reorder the interleaved chains, and the statistics kernels
        first[1] = min(first[1], (uint32_t)__shfl_xor((int)first[1], s, 64));           // missed the A/B rule with them: profiles/r20_header_refactor_ab.json)
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < kStatExt; ++e) { smEv[wave][e] = ev[e]; smEid[wave][e] = eid[e]; }
#pragma unroll
        for (int c = 0; c < kStatCnt; ++c) atomicAdd(&smCnt[c], cnt[c]);               // (cnt is wave-uniform: ballots)
        atomicMin(&smFirst[0], first[0]);
        atomicMin(&smFirst[1], first[1]);
    }
    __syncthreads();
    uint32_t* P = part + blockIdx.x;
    if (tid < kStatExt) {
        float v = smEv[0][tid];
        uint32_t id = smEid[0][tid];
        for (int w = 1; w < kBlock / 64; ++w) stat_take(stat_is_min(tid), v, id, smEv[w][tid], smEid[w][tid]);
        P[(size_t)tid * kStatGrid] = fbits(v);
        P[(size_t)(kStatExt + tid) * kStatGrid] = id;
    } else if (tid >= 64 && tid < 64 + kStatCnt) {
        P[(size_t)(2 * kStatExt + tid - 64) * kStatGrid] = smCnt[tid - 64];
    } else if (tid >= 128 && tid < 130) {
        P[(size_t)(2 * kStatExt + kStatCnt + tid - 128) * kStatGrid] = smFirst[tid - 128];
    }
    for (uint32_t i = tid; i < k.histWords; i += kBlock) tileHist[(size_t)blockIdx.x * k.histWords + i] = smHist[i];
}

// ---- cell occupancy from cellStart (numCells + 1 words) ------------------------------------------------------------------------
// Per block (a column of the slab): cells with 0 .. 63 and >= 64 members among its cells, then max over them of (count << 32) | (0xFFFFFFFF - cell).
__global__ __launch_bounds__(kBlock) void k_stats_cells(const uint32_t* __restrict__ cellStart, int numCells, unsigned long long* __restrict__ cellPart) {
    __shared__ uint32_t smOcc[65];
    __shared__ unsigned long long smMax;
    const int tid = threadIdx.x;
    if (tid < 65) smOcc[tid] = 0u;
    if (tid == 65) smMax = 0ull;
    __syncthreads();
    uint32_t zeros = 0u;
    unsigned long long best = 0ull;
    const int groups = (numCells + 3) / 4;                                             // four cells per thread and step: one 16-byte load + one word
    for (int q = blockIdx.x * kBlock + tid; q < groups; q += gridDim.x * kBlock) {
        const int c0 = 4 * q;
        uint32_t st[5];
        if (c0 + 4 <= numCells) {
            const uint4 v = *reinterpret_cast<const uint4*>(cellStart + c0);
            st[0] = v.x; st[1] = v.y; st[2] = v.z; st[3] = v.w; st[4] = cellStart[c0 + 4];
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) st[j] = cellStart[min(c0 + j, numCells)];      // (a repeated last word: a cell of 0 members, not counted below)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c0 + j >= numCells) break;
            const uint32_t m = st[j + 1] - st[j];
            if (m == 0u) ++zeros;
            else atomicAdd(&smOcc[min(m, 64u)], 1u);
            const unsigned long long key = ((unsigned long long)m << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(c0 + j));
            best = key > best ? key : best;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        zeros += (uint32_t)__shfl_xor((int)zeros, s, 64);
        const unsigned long long o = __shfl_xor(best, s, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) {
        atomicAdd(&smOcc[0], zeros);
        atomicMax(&smMax, best);
    }
    __syncthreads();
    if (tid < 65) cellPart[(size_t)tid * gridDim.x + blockIdx.x] = smOcc[tid];                 // column-major: k_stats_finish reads a column per step
    if (tid == 65) cellPart[(size_t)65 * gridDim.x + blockIdx.x] = smMax;
}

// ---- the tree over the tile sums (blocks 0 .. 14, one sum each), the blocks' partial records (block 15), the cells' rows (block 16) ----------
__global__ __launch_bounds__(kBlock) void k_stats_finish(StatK k, double* tileSums, const uint32_t* __restrict__ part,
                                                         const unsigned long long* __restrict__ cellPart, int nCellBlocks, SphStatistics* out) {
    __shared__ double smTree[kStatTreeLds];
    __shared__ float smEv[kBlock / 64][kStatExt];
    __shared__ uint32_t smEid[kBlock / 64][kStatExt];
    __shared__ unsigned long long smCnt[kStatCnt], smCell[kStatCellCols], smCellW[kBlock / 64][kStatCellCols];
    __shared__ uint32_t smFirst[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T2 = k.tilesPow2;
    if (blockIdx.x < kStatSums) {
        // tile sums padded with +0.0 to T2, then x[i] += x[i + s] for s = T2 / 2 .. 1 (one block, so a barrier orders the steps)
        const int s = blockIdx.x;
        double* x = tileSums + (size_t)s * T2;
        double total;
        if (T2 <= kStatTreeLds) {
#pragma unroll 8
            for (int i = tid; i < T2; i += kBlock) smTree[i] = i < k.nTiles ? x[i] : 0.0;                 // (unrolled: the loads leave together)
            __syncthreads();
            for (int h = T2 >> 1; h >= 1; h >>= 1) {
                for (int i = tid; i < h; i += kBlock) smTree[i] = smTree[i] + smTree[i + h];
                __syncthreads();
            }
            total = smTree[0];
        } else {
            for (int i = k.nTiles + tid; i < T2; i += kBlock) x[i] = 0.0;
            __threadfence_block();
            __syncthreads();
            for (int h = T2 >> 1; h >= 1; h >>= 1) {
                for (int i = tid; i < h; i += kBlock) x[i] = x[i] + x[i + h];
                __threadfence_block();
                __syncthreads();
            }
            total = x[0];
        }
        if (tid == 0) {
            double* dst = s < 3 ? &out->sumPos[s] : s < 6 ? &out->sumVel[s - 3] : s == 6 ? &out->sumSpeed2 : s == 7 ? &out->sumDensity : s == 8 ? &out->sumDensity2
                        : s == 9 ? &out->sumPressure : s == 10 ? &out->sumFoam : s == 11 ? &out->sumInvDensity : &out->sumAngular[s - 12];
            *dst = total;
        }
    } else if (blockIdx.x == kStatSums) {
        if (tid < kStatCnt) smCnt[tid] = 0ull;
        if (tid < 2) smFirst[tid] = 0xFFFFFFFFu;
        __syncthreads();
        float ev[kStatExt];
        uint32_t eid[kStatExt], first[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        unsigned long long cnt[kStatCnt];
#pragma unroll
        for (int e = 0; e < kStatExt; ++e) { ev[e] = stat_is_min(e) ? INFINITY : -INFINITY; eid[e] = 0xFFFFFFFFu; }
#pragma unroll
        for (int c = 0; c < kStatCnt; ++c) cnt[c] = 0ull;
#pragma unroll 2
        for (int t = tid; t < k.nBlocks; t += kBlock) {
            const uint32_t* P = part + t;
#pragma unroll
            for (int e = 0; e < kStatExt; ++e)
                stat_take(stat_is_min(e), ev[e], eid[e], bitsf(P[(size_t)e * kStatGrid]), P[(size_t)(kStatExt + e) * kStatGrid]);
#pragma unroll
            for (int c = 0; c < kStatCnt; ++c) cnt[c] += P[(size_t)(2 * kStatExt + c) * kStatGrid];
            first[0] = min(first[0], P[(size_t)(2 * kStatExt + kStatCnt) * kStatGrid]);
            first[1] = min(first[1], P[(size_t)(2 * kStatExt + kStatCnt + 1) * kStatGrid]);
        }
        stat_wave_ext(ev, eid);
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int c = 0; c < kStatCnt; ++c) cnt[c] += __shfl_xor(cnt[c], s, 64);
            first[0] = min(first[0], (uint32_t)__shfl_xor((int)first[0], s, 64));
            first[1] = min(first[1], (uint32_t)__shfl_xor((int)first[1], s, 64));
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kStatExt; ++e) { smEv[wave][e] = ev[e]; smEid[wave][e] = eid[e]; }
#pragma unroll
            for (int c = 0; c < kStatCnt; ++c) atomicAdd(&smCnt[c], cnt[c]);
            atomicMin(&smFirst[0], first[0]);
            atomicMin(&smFirst[1], first[1]);
        }
        __syncthreads();
        if (tid < kStatExt) {
            float v = smEv[0][tid];
            uint32_t id = smEid[0][tid];
            for (int w = 1; w < kBlock / 64; ++w) stat_take(stat_is_min(tid), v, id, smEv[w][tid], smEid[w][tid]);
            SphStatExtremum* dst = tid < 3 ? &out->minPos[tid] : tid < 6 ? &out->maxPos[tid - 3] : tid == 6 ? &out->minDensity : tid == 7 ? &out->maxDensity
                                 : tid == 8 ? &out->minPressure : tid == 9 ? &out->maxPressure : tid == 10 ? &out->maxFoam : &out->maxSpeed2;
            dst->value = v;
            dst->id = id;
            if (tid == 11) {
                out->maxSpeed = id == 0xFFFFFFFFu ? 0.0f : sqrtf(v);
                out->reserved0 = 0u;
            }
        }
        if (tid == 64) {
            out->numRecords = (unsigned long long)k.n;
            out->numFluid = smCnt[0];
            out->numActiveGhosts = smCnt[1];
            out->numInactiveGhosts = smCnt[2];
            out->numOther = smCnt[3];
            out->numNonFinite = smCnt[4];
            out->numCounted = smCnt[5];
            out->numEscaped = smCnt[6];
            out->firstNonFiniteId = smFirst[0];
            out->firstEscapedId = smFirst[1];
        }
    } else {
        // thread = row (nCellBlocks <= kBlock), one coalesced load per column, a wave reduction each, then the four waves
        // (22 columns at a time: their loads leave together, then the reductions)
        for (int c0 = 0; c0 < kStatCellCols; c0 += 22) {
            unsigned long long v[22];
#pragma unroll
            for (int j = 0; j < 22; ++j) v[j] = tid < nCellBlocks ? cellPart[(size_t)(c0 + j) * nCellBlocks + tid] : 0ull;
#pragma unroll
            for (int j = 0; j < 22; ++j) {
                for (int s = 32; s >= 1; s >>= 1) {
                    const unsigned long long o = __shfl_xor(v[j], s, 64);
                    v[j] = c0 + j == 65 ? (o > v[j] ? o : v[j]) : v[j] + o;
                }
                if (lane == 0) smCellW[wave][c0 + j] = v[j];
            }
        }
        __syncthreads();
        if (tid < kStatCellCols) {
            unsigned long long v = smCellW[0][tid];
            for (int w = 1; w < kBlock / 64; ++w) v = tid == 65 ? (smCellW[w][tid] > v ? smCellW[w][tid] : v) : v + smCellW[w][tid];
            smCell[tid] = v;
        }
        __syncthreads();
        if (tid < 65) out->occupancy[tid] = smCell[tid];
        if (tid == 65) {
            out->occupiedCells = (unsigned long long)k.numCells - smCell[0];
            out->maxCellCount = (uint32_t)(smCell[65] >> 32);
            out->maxCellIndex = 0xFFFFFFFFu - (uint32_t)(smCell[65] & 0xFFFFFFFFull);
        }
    }
}

// ---- histogram rows of the blocks -> 64-bit counters: 4 bins per block, 64 groups of rows per bin ----------------------------------------
constexpr int kStatHistBins = 4;
__global__ __launch_bounds__(kBlock) void k_stats_hist(const uint32_t* __restrict__ tileHist, int nRows, uint32_t histWords, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sm[kBlock / kStatHistBins][kStatHistBins + 1];
    const int b = threadIdx.x % kStatHistBins, g = threadIdx.x / kStatHistBins;
    const uint32_t bin = blockIdx.x * (uint32_t)kStatHistBins + (uint32_t)b;
    unsigned long long s = 0ull;
    if (bin < histWords) {
#pragma unroll 8
        for (int t = g; t < nRows; t += kBlock / kStatHistBins) s += tileHist[(size_t)t * histWords + bin];
    }
    sm[g][b] = s;
    __syncthreads();
    if (threadIdx.x < kStatHistBins && bin < histWords) {
        unsigned long long tot = 0ull;
        for (int j = 0; j < kBlock / kStatHistBins; ++j) tot += sm[j][b];
        out[bin] = tot;
    }
}

}  // namespace sph
