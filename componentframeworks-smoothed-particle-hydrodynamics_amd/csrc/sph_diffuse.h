// sph_diffuse.h -- spray, foam and bubbles: secondary particles spawned by the fluid (no reference counterpart).
//
// A pool of up to C 48-byte records (three float4: pos, life | vel, age | parent, birth, kind, pad) that do not act on the fluid.  One
// substep, on the sorted copy of the substep's ENTRY state (the grid dispatch_one has just built for the SPH pass):
//   k_diffuse_advance   one living record per lane: u and the neighbour count n of the Shepard field at its position (tracer_field: the
//                       sampler's candidates in the sampler's order), class by n, move by class, age, death test.  The advanced record
//                       goes to the SCRATCH pool at the same index, a 0 / 1 survivor flag beside it, and the block's seven counts
//                       (four causes of death, three classes of survivors) to its row of part[]
//   k_diffuse_count     one sorted slot per lane: the number of children of that fluid particle, stored at cnt[id] -- id order, not slot
//                       order, so nothing depends on the cell sort
//   (scan)              the engine's scan kernels over the flags (C) and over the child counts (N)
//   k_diffuse_compact   scratch record i -> pool[flagStart[i]] if it survived: stable compaction back into the pool the next substep reads
//   k_diffuse_emit      one sorted slot per lane: child k of parent id -> pool[survivors + cntStart[id] + k] while that is below C
//   k_diffuse_tick      one block behind them: adds up part[], then its thread 0 advances the 64-bit substep counter, the alive count and
//                       the running totals (device memory, because a captured graph bakes its launch arguments in)
// No float atomics, no integer atomics either; every launch is sized by C or N; every index derived from a device-side count is clamped
// to C.  Every fp32 expression is a multiply, then an add (-ffp-contract=off: no fma); diffuse_move / diffuse_children / diffuse_child are
// __host__ __device__ so that sph_diffuse_step_host runs the same statements.
//
// Crest births (the optional second birth term, sph_abi.h SphDiffuseCrest): the engine runs a free-surface pass by slot over the same
// grid (sph_shell.h; this header does not include it) and hands its plain arrays to
//   k_diffuse_count_crest  k_diffuse_count plus diffuse_crest_children from the slot's normal, crest sum and sorted velocity on an acting
//                          substep; the block's crest children go to its row of crestPart[]
//   k_diffuse_crest_tick   one block in front of k_diffuse_tick (which advances the counter): adds up crestPart[], then its thread 0
//                          advances the crest books
// diffuse_crest_children takes plain scalars and is __host__ __device__: sph_diffuse_step_host_crest runs it on SphShell rows.
#pragma once
#include "sph_tracer.h"   // built on the tracer's field sample: tracer_field

namespace sph {

// The coefficients as the kernels read them (device memory: a replayed graph sees a later change).
struct DiffuseCoef {
    float threshold, rate, lifeMin, lifeMax, spread, kb, kd, maxAge;
    uint32_t sprayBelow, bubbleAbove, maxPerParent, seed;
};

// state[] words (uint32)
enum : int {
    DF_ALIVE = 0, DF_STEP_LO = 1, DF_STEP_HI = 2, DF_CLASS = 3 /* 3 words */,
    DF_TOTALS = 6 /* 7 x (lo, hi): spawned, dropped, died by life, by age, left the box, non-finite, seeded */, DF_WORDS = 20
};
enum : int { DF_PART_LIFE = 0, DF_PART_AGE = 1, DF_PART_BOX = 2, DF_PART_NONFINITE = 3, DF_PART_CLASS = 4, DF_PART_WORDS = 8 };
enum : uint32_t { DF_SPRAY = 0u, DF_FOAM = 1u, DF_BUBBLE = 2u };
enum : int { DF_LIVES = 0, DF_DIED_LIFE = 1, DF_DIED_AGE = 2, DF_DIED_BOX = 3, DF_DIED_NONFINITE = 4 };

struct DiffuseRec {
    float px, py, pz, life, vx, vy, vz, age;
    uint32_t parent, birth, kind, pad;
};
struct DiffuseBox { float lo[3], hi[3]; float gx, gy, gz; };   // the grid's box and the params' gravity

// ---- the counter-based hash: no state is carried, nothing depends on thread order ----
__host__ __device__ inline uint32_t diffuse_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t diffuse_hash(uint32_t seed, uint32_t id, uint32_t stepLo, uint32_t stepHi, uint32_t draw) {
    uint32_t h = diffuse_mix(seed + 0x9e3779b9u);
    h = diffuse_mix(h ^ id);
    h = diffuse_mix(h ^ stepLo);
    h = diffuse_mix(h ^ stepHi);
    return diffuse_mix(h ^ draw);
}
// a uniform in [0, 1): 24 bits, exact in fp32
__host__ __device__ inline float diffuse_uniform(uint32_t seed, uint32_t id, uint32_t stepLo, uint32_t stepHi, uint32_t draw) {
    return (float)(diffuse_hash(seed, id, stepLo, stepHi, draw) >> 8) * 5.9604644775390625e-08f;
}

__host__ __device__ inline bool diffuse_isfinite(float x) { return x - x == 0.0f; }

// One record's substep from its sample (u, n): the new record and what became of it (DF_LIVES or the cause of death, in the order
// non-finite, box, life, age).
__host__ __device__ inline int diffuse_move(const DiffuseCoef& c, const DiffuseBox& b, float dt, float ux, float uy, float uz, uint32_t n, DiffuseRec& r) {
    float vx, vy, vz;
    if (n < c.sprayBelow) {
        r.kind = DF_SPRAY;
        vx = r.vx + dt * b.gx; vy = r.vy + dt * b.gy; vz = r.vz + dt * b.gz;
    } else if (n > c.bubbleAbove) {
        r.kind = DF_BUBBLE;
        const float dk = dt * c.kb;
        vx = (r.vx - dk * b.gx) + c.kd * (ux - r.vx);
        vy = (r.vy - dk * b.gy) + c.kd * (uy - r.vy);
        vz = (r.vz - dk * b.gz) + c.kd * (uz - r.vz);
    } else {
        r.kind = DF_FOAM;
        vx = ux; vy = uy; vz = uz;
        r.life = r.life - dt;
    }
    r.px = r.px + dt * vx; r.py = r.py + dt * vy; r.pz = r.pz + dt * vz;
    r.vx = vx; r.vy = vy; r.vz = vz;
    r.age = r.age + dt;
    if (!(diffuse_isfinite(r.px) && diffuse_isfinite(r.py) && diffuse_isfinite(r.pz))) return DF_DIED_NONFINITE;
    if (r.px < b.lo[0] || r.px > b.hi[0] || r.py < b.lo[1] || r.py > b.hi[1] || r.pz < b.lo[2] || r.pz > b.hi[2]) return DF_DIED_BOX;
    if (!(r.life > 0.0f)) return DF_DIED_LIFE;
    if (r.age > c.maxAge) return DF_DIED_AGE;
    return DF_LIVES;
}

// Children of a fluid particle this substep.  flags: F_* of sph_device.h; invRho: the sorted copy's 1/rho (0 for density <= 0).
__host__ __device__ inline uint32_t diffuse_children(const DiffuseCoef& c, float dt, float foam, uint32_t flags, float invRho, uint32_t id,
                                                     uint32_t stepLo, uint32_t stepHi) {
    if (flags & F_GHOSTNZ) return 0u;                                   // (fluid is isGhost == 0; isActive means something for ghosts only and the spawners write 0)
    if (!(invRho > 0.0f)) return 0u;
    if (!diffuse_isfinite(foam) || !(foam > c.threshold)) return 0u;
    const float rd = c.rate * dt;
    const float lam = rd * (foam - c.threshold);
    const float f = floorf(lam + diffuse_uniform(c.seed, id, stepLo, stepHi, 0u));
    if (!(f < (float)c.maxPerParent)) return c.maxPerParent;
    return f > 0.0f ? (uint32_t)f : 0u;
}

// ---- crest births ----
// The coefficients of the crest term as the kernels read them (device memory, beside DiffuseCoef: a replayed graph sees a later change).
struct DiffuseCrestCoef {
    float rate, crestMin, crestMax, speedMin, speedMax, align;
    uint32_t every, pad;
};
// crest[] words (uint32): the books of the crest term
enum : int { DFC_ACTING = 0 /* (lo, hi) */, DFC_SPAWNED = 2 /* (lo, hi) */, DFC_SHELL = 4, DFC_WORDS = 8 };

// Does the term act on the substep whose counter, before the step, is (lo, hi)?
__host__ __device__ inline bool diffuse_crest_acts(uint32_t lo, uint32_t hi, uint32_t every) {
    return every != 0u && (((unsigned long long)hi << 32) | lo) % every == 0ull;
}
__host__ __device__ inline float diffuse_window(float x, float lo, float hi) { return fminf(fmaxf((x - lo) / (hi - lo), 0.0f), 1.0f); }

// Children of the crest term of a fluid particle on an acting substep, before the cap on the sum with the foam term's.  (nx, ny, nz),
// crest, member, isolated: the particle's free-surface row; (vx, vy, vz): its velocity.  Draw 33: the first draw diffuse_child leaves.
__host__ __device__ inline uint32_t diffuse_crest_children(const DiffuseCoef& c, const DiffuseCrestCoef& cc, float dt, uint32_t flags, float invRho,
                                                           bool member, bool isolated, float nx, float ny, float nz, float crest,
                                                           float vx, float vy, float vz, uint32_t id, uint32_t stepLo, uint32_t stepHi) {
    if (flags & F_GHOSTNZ) return 0u;
    if (!(invRho > 0.0f)) return 0u;
    if (!member || isolated) return 0u;
    const float sp2 = dot3(vx, vy, vz, vx, vy, vz);
    if (!diffuse_isfinite(sp2)) return 0u;
    const float sp = sqrtf(sp2);
    if (!(sp > 0.0f)) return 0u;
    if (!(dot3(vx, vy, vz, nx, ny, nz) >= cc.align * sp)) return 0u;
    const float pc = diffuse_window(crest, cc.crestMin, cc.crestMax);
    const float pk = diffuse_window(sp, cc.speedMin, cc.speedMax);
    const float p = pc * pk;
    if (!(p > 0.0f)) return 0u;
    const float lam = ((cc.rate * dt) * (float)cc.every) * p;
    const float f = floorf(lam + diffuse_uniform(c.seed, id, stepLo, stepHi, 33u));
    if (!(f < (float)c.maxPerParent)) return c.maxPerParent;
    return f > 0.0f ? (uint32_t)f : 0u;
}

// Child k of parent id: draws 1 + 4 k .. 4 + 4 k.
__host__ __device__ inline DiffuseRec diffuse_child(const DiffuseCoef& c, float h, float px, float py, float pz, float vx, float vy, float vz,
                                                    uint32_t id, uint32_t stepLo, uint32_t stepHi, uint32_t k) {
    const float sh = c.spread * h;
    const uint32_t d0 = 1u + 4u * k;
    DiffuseRec r;
    r.px = px + sh * (2.0f * diffuse_uniform(c.seed, id, stepLo, stepHi, d0) - 1.0f);
    r.py = py + sh * (2.0f * diffuse_uniform(c.seed, id, stepLo, stepHi, d0 + 1u) - 1.0f);
    r.pz = pz + sh * (2.0f * diffuse_uniform(c.seed, id, stepLo, stepHi, d0 + 2u) - 1.0f);
    r.life = c.lifeMin + diffuse_uniform(c.seed, id, stepLo, stepHi, d0 + 3u) * (c.lifeMax - c.lifeMin);
    r.vx = vx; r.vy = vy; r.vz = vz;
    r.age = 0.0f;
    r.parent = id; r.birth = stepLo; r.kind = DF_FOAM; r.pad = 0u;
    return r;
}

__host__ __device__ inline DiffuseBox diffuse_box(const float gmin[3], float cellSize, const int dims[3], float gx, float gy, float gz) {
    DiffuseBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = gmin[a]; b.hi[a] = gmin[a] + (float)dims[a] * cellSize; }
    b.gx = gx; b.gy = gy; b.gz = gz;
    return b;
}

__device__ __forceinline__ DiffuseBox diffuse_box_of(const SimK& k) {
    const float gmin[3] = {k.gminx, k.gminy, k.gminz};
    const int dims[3] = {k.gx, k.gy, k.gz};
    return diffuse_box(gmin, k.cellSize, dims, k.gravx, k.gravy, k.gravz);
}

__device__ __forceinline__ uint32_t diffuse_alive(const uint32_t* __restrict__ state, uint32_t C) { return min(state[DF_ALIVE], C); }

// ---- advance: pool -> scratch (same index), flag, per-block counts ----
__global__ __launch_bounds__(kBlock) void k_diffuse_advance(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart, float dt,
                                                            const DiffuseCoef* __restrict__ coef, const uint32_t* __restrict__ state,
                                                            const float4* __restrict__ pool, float4* __restrict__ scratch,
                                                            uint32_t* __restrict__ flag, uint32_t* __restrict__ part, uint32_t C) {
    __shared__ uint32_t sm[4][DF_PART_WORDS];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t alive = diffuse_alive(state, C);
    int fate = -1, kind = -1;
    if (i < alive) {
        const DiffuseCoef c = *coef;
        const float4 a = pool[(size_t)3 * i], b = pool[(size_t)3 * i + 1u], w = pool[(size_t)3 * i + 2u];
        DiffuseRec r{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, fbits(w.x), fbits(w.y), fbits(w.z), fbits(w.w)};
        const SampleOut o = tracer_field(k, pv, cellStart, a.x, a.y, a.z);      // (all zero for a non-finite position)
        fate = diffuse_move(c, diffuse_box_of(k), dt, o.vx, o.vy, o.vz, o.count, r);
        kind = (int)r.kind;
        scratch[(size_t)3 * i] = make_float4(r.px, r.py, r.pz, r.life);
        scratch[(size_t)3 * i + 1u] = make_float4(r.vx, r.vy, r.vz, r.age);
        scratch[(size_t)3 * i + 2u] = make_float4(bitsf(r.parent), bitsf(r.birth), bitsf(r.kind), bitsf(r.pad));
        flag[i] = fate == DF_LIVES ? 1u : 0u;
    }
    // the block's counts: a ballot per counter, one row per wave in LDS, one row per block in memory
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t mine = 0u;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const bool hit = q < 4 ? fate == q + 1 : (fate == DF_LIVES && kind == q - 4);
        const uint32_t cnt = (uint32_t)__popcll(__ballot(hit));
        if (lane == q) mine = cnt;
    }
    if (lane < DF_PART_WORDS) sm[wv][lane] = mine;
    __syncthreads();
    if (threadIdx.x < DF_PART_WORDS)
        part[(size_t)blockIdx.x * DF_PART_WORDS + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

// ---- child counts over the sorted slots, stored in id order ----
__global__ __launch_bounds__(kBlock) void k_diffuse_count(const float4* __restrict__ pv, const float4* __restrict__ own, float dt,
                                                          const DiffuseCoef* __restrict__ coef, const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ cnt, uint32_t idBase, uint32_t n) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const float4 o = own[s];                                            // (cell, foam, flags, id)
    const uint32_t idx = fbits(o.w) - idBase;
    if (idx >= n) return;                                               // (never: ids are idBase + [0, n))
    cnt[idx] = diffuse_children(*coef, dt, o.y, fbits(o.z), pv[2u * s].w, fbits(o.w), state[DF_STEP_LO], state[DF_STEP_HI]);
}

// ---- child counts with the crest term: nrmSlot (normal, 0 outside the shell | 1 member | 2 isolated member) and crestSlot are by slot ----
__global__ __launch_bounds__(kBlock) void k_diffuse_count_crest(const float4* __restrict__ pv, const float4* __restrict__ own, float dt,
                                                                const DiffuseCoef* __restrict__ coef, const DiffuseCrestCoef* __restrict__ crestCoef,
                                                                const uint32_t* __restrict__ state, const float4* __restrict__ nrmSlot,
                                                                const float* __restrict__ crestSlot, uint32_t* __restrict__ cnt,
                                                                uint32_t* __restrict__ crestPart, uint32_t idBase, uint32_t n) {
    __shared__ uint32_t sm[4];
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    uint32_t extra = 0u;
    if (s < n) {
        const float4 o = own[s];                                        // (cell, foam, flags, id)
        const uint32_t idx = fbits(o.w) - idBase;
        if (idx < n) {                                                  // (always: ids are idBase + [0, n))
            const DiffuseCoef c = *coef;
            const DiffuseCrestCoef cc = *crestCoef;
            const uint32_t lo = state[DF_STEP_LO], hi = state[DF_STEP_HI];
            const float invRho = pv[2u * s].w;
            const uint32_t f = diffuse_children(c, dt, o.y, fbits(o.z), invRho, fbits(o.w), lo, hi);
            uint32_t all = f;
            if (f < c.maxPerParent && diffuse_crest_acts(lo, hi, cc.every)) {   // (a full parent has no room for a crest child: nothing is read)
                const float4 N = nrmSlot[s], V = pv[2u * s + 1u];
                const uint32_t born = diffuse_crest_children(c, cc, dt, fbits(o.z), invRho, N.w != 0.0f, N.w == 2.0f, N.x, N.y, N.z, crestSlot[s],
                                                             V.x, V.y, V.z, fbits(o.w), lo, hi);
                all = min(f + born, c.maxPerParent);
            }
            extra = all - f;
            cnt[idx] = all;
        }
    }
    uint32_t total;
    (void)block_excl_scan(extra, sm, total);
    if (threadIdx.x == 0) crestPart[blockIdx.x] = total;
}

// ---- stable compaction of the survivors: scratch -> pool ----
__global__ __launch_bounds__(kBlock) void k_diffuse_compact(const float4* __restrict__ scratch, const uint32_t* __restrict__ flagStart,
                                                            const uint32_t* __restrict__ state, float4* __restrict__ pool, uint32_t C) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= diffuse_alive(state, C)) return;
    const uint32_t d = flagStart[i];
    if (flagStart[i + 1u] == d || d >= C) return;                      // died (d < C always: d <= i)
    pool[(size_t)3 * d] = scratch[(size_t)3 * i];
    pool[(size_t)3 * d + 1u] = scratch[(size_t)3 * i + 1u];
    pool[(size_t)3 * d + 2u] = scratch[(size_t)3 * i + 2u];
}

// ---- the newborn, behind the survivors in (parent id, k) order ----
__global__ __launch_bounds__(kBlock) void k_diffuse_emit(SimK k, const float4* __restrict__ pv, const float4* __restrict__ own,
                                                         const DiffuseCoef* __restrict__ coef, const uint32_t* __restrict__ state,
                                                         const uint32_t* __restrict__ cntStart, const uint32_t* __restrict__ flagStart,
                                                         float4* __restrict__ pool, uint32_t idBase, uint32_t n, uint32_t C) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t id = fbits(own[s].w), idx = id - idBase;
    if (idx >= n) return;
    const uint32_t first = cntStart[idx], children = min(cntStart[idx + 1u] - first, 8u);
    if (children == 0u) return;
    const uint32_t survivors = min(flagStart[C], C);
    const uint32_t room = C - survivors;                                // newborn that fit
    if (first >= room) return;
    const DiffuseCoef c = *coef;
    const float4 P = pv[2u * s], V = pv[2u * s + 1u];
    const uint32_t lo = state[DF_STEP_LO], hi = state[DF_STEP_HI];
    for (uint32_t q = 0; q < children && first + q < room; ++q) {
        const DiffuseRec r = diffuse_child(c, k.h, P.x, P.y, P.z, V.x, V.y, V.z, id, lo, hi, q);
        const uint32_t d = survivors + first + q;                       // (< C: first + q < room)
        pool[(size_t)3 * d] = make_float4(r.px, r.py, r.pz, r.life);
        pool[(size_t)3 * d + 1u] = make_float4(r.vx, r.vy, r.vz, r.age);
        pool[(size_t)3 * d + 2u] = make_float4(bitsf(r.parent), bitsf(r.birth), bitsf(r.kind), bitsf(r.pad));
    }
}

__device__ __forceinline__ void diffuse_add64(uint32_t* w, unsigned long long v) {
    const unsigned long long t = (((unsigned long long)w[1] << 32) | w[0]) + v;
    w[0] = (uint32_t)t; w[1] = (uint32_t)(t >> 32);
}

// ---- one block: the rows of part[] added up, then thread 0 alone writes the state ----
__global__ __launch_bounds__(kBlock) void k_diffuse_tick(uint32_t* __restrict__ state, const uint32_t* __restrict__ part, uint32_t rows,
                                                         const uint32_t* __restrict__ flagStart, const uint32_t* __restrict__ cntStart, uint32_t n, uint32_t C) {
    __shared__ uint32_t sm[DF_PART_WORDS][4];
    __shared__ uint32_t tot[DF_PART_WORDS];
    const uint32_t usedRows = min(rows, (diffuse_alive(state, C) + (uint32_t)kBlock - 1u) / (uint32_t)kBlock);   // (rows behind the living records hold zeros anyway)
    uint32_t acc[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t r = threadIdx.x; r < usedRows; r += kBlock)
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[q] += part[(size_t)r * DF_PART_WORDS + q];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        uint32_t t;
        (void)block_excl_scan(acc[q], sm[q], t);
        if (threadIdx.x == 0) tot[q] = t;
    }
    __syncthreads();
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const uint32_t survivors = min(flagStart[C], C);
    const uint32_t spawned = cntStart[n];
    const uint32_t born = min(spawned, C - survivors);
    state[DF_ALIVE] = survivors + born;
    state[DF_CLASS + 0] = tot[DF_PART_CLASS + 0];
    state[DF_CLASS + 1] = tot[DF_PART_CLASS + 1] + born;               // the newborn are foam until their first substep classes them
    state[DF_CLASS + 2] = tot[DF_PART_CLASS + 2];
    diffuse_add64(state + DF_TOTALS + 0, spawned);
    diffuse_add64(state + DF_TOTALS + 2, spawned - born);
    diffuse_add64(state + DF_TOTALS + 4, tot[DF_PART_LIFE]);
    diffuse_add64(state + DF_TOTALS + 6, tot[DF_PART_AGE]);
    diffuse_add64(state + DF_TOTALS + 8, tot[DF_PART_BOX]);
    diffuse_add64(state + DF_TOTALS + 10, tot[DF_PART_NONFINITE]);
    diffuse_add64(state + DF_STEP_LO, 1ull);
}

// ---- one block in front of k_diffuse_tick: the rows of crestPart[] added up, then thread 0 alone writes the crest books ----
// shellTotal: the word behind the scan of the shell flags by slot (the number of shell members), clamped to n.
__global__ __launch_bounds__(kBlock) void k_diffuse_crest_tick(const uint32_t* __restrict__ state, const DiffuseCrestCoef* __restrict__ crestCoef,
                                                               const uint32_t* __restrict__ crestPart, uint32_t rows,
                                                               const long long* __restrict__ shellTotal, uint32_t n, uint32_t* __restrict__ crest) {
    __shared__ uint32_t sm[4];
    uint32_t acc = 0u;
    for (uint32_t r = threadIdx.x; r < rows; r += kBlock) acc += crestPart[r];
    uint32_t total;
    (void)block_excl_scan(acc, sm, total);
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    if (!diffuse_crest_acts(state[DF_STEP_LO], state[DF_STEP_HI], crestCoef->every)) return;
    const long long t = n ? *shellTotal : 0ll;
    diffuse_add64(crest + DFC_ACTING, 1ull);
    diffuse_add64(crest + DFC_SPAWNED, total);
    crest[DFC_SHELL] = t < 0ll ? 0u : (t > (long long)n ? n : (uint32_t)t);
}

}  // namespace sph
