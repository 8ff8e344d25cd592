// sph_wave.h -- wave (64 lanes) and block (256 threads = 4 waves) primitives: scans and reductions, stated once for every header.
// Base layer: it uses nothing of the project.  Every lane of the wave (every thread of the block) must arrive at a call.
//   wave_incl_scan[64] / block_excl_scan[64]   inclusive prefix sum across the wave / exclusive across the block with the block's sum (sm: 4 words of LDS)
//   wave_sum / wave_min / wave_max        the value of the whole wave in every lane; the butterfly runs 32, 16, ..., 1 for every type, so a
//                                         float or double sum has one fixed order (and its bits) wherever it is taken
//   block_max                             the largest value of the block in every thread; sm: 4 words of LDS
//   wave_append                           compaction: one record per lane with a predicate, appended behind a device counter with one atomic per wave
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sph {

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_incl_scan64(unsigned long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// block-wide exclusive scan of one value per thread (256 threads = 4 waves); returns the exclusive prefix and, through total, the block sum.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sm, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    uint32_t w0 = sm[0], w1 = sm[1], w2 = sm[2], w3 = sm[3];
    uint32_t base = (w > 0 ? w0 : 0u) + (w > 1 ? w1 : 0u) + (w > 2 ? w2 : 0u);
    total = w0 + w1 + w2 + w3;
    __syncthreads();
    return base + inc - v;
}
__device__ __forceinline__ unsigned long long block_excl_scan64(unsigned long long v, unsigned long long* sm, unsigned long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long inc = wave_incl_scan64(v);
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    const unsigned long long w0 = sm[0], w1 = sm[1], w2 = sm[2], w3 = sm[3];
    const unsigned long long base = (w > 0 ? w0 : 0ull) + (w > 1 ? w1 : 0ull) + (w > 2 ? w2 : 0ull);
    total = w0 + w1 + w2 + w3;
    __syncthreads();
    return base + inc - v;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) { for (int sh = 32; sh >= 1; sh >>= 1) v = v + __shfl_xor(v, sh, 64); return v; }
template <class T>
__device__ __forceinline__ T wave_min(T v) {
    for (int sh = 32; sh >= 1; sh >>= 1) { const T o = __shfl_xor(v, sh, 64); v = v > o ? o : v; }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    for (int sh = 32; sh >= 1; sh >>= 1) { const T o = __shfl_xor(v, sh, 64); v = v < o ? o : v; }
    return v;
}

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* sm) {
    for (int sh = 32; sh >= 1; sh >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, sh, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    __syncthreads();
    return m;
}

// Wave-aggregated append: the lanes with pred take consecutive slots of buf behind *counter (one atomicAdd per wave, by its first such lane) and
// store rec there if the slot is below cap; *counter counts every lane with pred, stored or not.  Lanes without pred only take part in the ballot.
template <class R>
__device__ __forceinline__ void wave_append(R* buf, uint32_t* counter, uint32_t cap, bool pred, const R& rec) {
    const unsigned long long m = __ballot(pred);
    if (!pred) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (slot < cap) buf[slot] = rec;
}

}  // namespace sph
