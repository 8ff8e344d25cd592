// sph_shell.h -- free-surface particles: which particles (or query points) lie in the outer shell of the fluid, which way the surface
// faces there, and how sharply convex it is (no reference counterpart).
//
// Grid, radius rules, stencil, candidates and the target of a lane are those of sph_query.h (neighbor_stencil, neighbor_rows,
// query_target, neighbor_offset, neighbor_gather).
// Only positions enter.  Pass 1 sums, over the accepted candidates j of a target at x in row order, with d = x_j - x, t = R2 - r2 and
// w = t * t:  cnt += 1, W += w, S = fma(w, d, S).  The finish turns (cnt, W, S) into the record: s2 = dot3(S, S), lim = (offset R) W,
// in the shell iff cnt == 0 or cnt < minCount or s2 > lim^2; normal = -S / sqrt(s2) (zero where s2 == 0); offsetRatio = sqrt(s2) /
// (R W) (zero where W == 0).  Pass 2 runs for shell particles only and counts shell candidates only: where dot(d, n_i) < 0 (the
// candidate lies behind the target's tangent plane), the term (1 - dot(n_i, n_j)) (1 - sqrt(r2) / R) joins the crest sum, which is
// kept in fixed point (units of 2^-32) so that it is the same whatever the order of the candidates.
//
//   shell_add / shell_finish / shell_crest_term / shell_crest_value   __host__ __device__: sph_shell_host runs the same functions over
//                             HostGrid in the same row order, so the device's rows equal the twin's bytes.  sqrtf and the divisions
//                             are correctly rounded on both sides (hipcc's defaults, as sph_rays.h relies on them); everything else is
//                             the explicit fmaf()s and single operations (-ffp-contract=off).
// Two bodies, four kernels:
//   shell_row<SKIP>           pass 1 of one target: the zero row, or neighbor_gather (candidate positions straight from global memory,
//                             16 B each) into lane-owned sums and shell_finish.
//   shell_crest_sum           pass 2 of one shell slot; a candidate that is not in the shell costs the one 16-byte load of its by-slot
//                             float4 (read before the position: the loop is its own).
//   k_shell_gather<P>         pass 1 per lane (P: sorted-slot order, rows numbered by id, own slot skipped; else the caller's points) with
//                             shell_row's text written out: through shell_row it measured 2.2 to 2.5 % slower, with two more scalar
//                             instructions in front of an unchanged loop (profiles/r23_shell_walk_ab.json).  Writes the 32-byte row, the by-row flag word for the scan of ids[], and for particles the by-slot float4
//                             (normal, shell ? 1 : 0) and the by-slot flag word; adds (isolated rows, largest count) to stats with one
//                             integer atomic per wave and word.
//   k_shell_crest             shell_crest_sum over the compacted shell slots in ascending slot order (full waves whose lanes still share
//                             rows); writes the crest of the row by id.
//   k_shell_slot_gather /     the same bodies by slot for a substep that reads them itself (the diffuse pool's crest births): 20 bytes
//   k_shell_slot_crest        per target instead of 56, one float per slot, no rows by id, no atomics, both sized by n and gated by a
//                             counter in device memory (shell_gate)
//   k_shell_compact           (sph_query.h) out[offsets[i]] = i where flag[i]: the scan's second half, used twice (ids[] by row, shell
//                             slots by slot).
// ids[] is k_neighbors_ids' (a permutation of [0, n)); the range guards (row < rows, j < end <= n, offsets < rows) stay so that no load
// or store can leave its array.
#pragma once
#include <math.h>

#include "sph_query.h"

namespace sph {

constexpr int kShellFluidOnly = 1;                    // SPH_SHELL_FLUID_ONLY of sph_abi.h
constexpr uint32_t kShellMember = 1u, kShellIsolated = 2u;   // SPH_SHELL_MEMBER, SPH_SHELL_ISOLATED: flags of a row

struct ShellRow {                                     // SphShell of sph_abi.h
    float normal[3];
    float offsetRatio, crest;
    uint32_t count, flags, pad;
};
static_assert(sizeof(ShellRow) == 32, "SphShell is 32 bytes");

struct ShellAcc {
    uint32_t cnt;
    float W, Sx, Sy, Sz;
};
__host__ __device__ inline void shell_reset(ShellAcc& a) { a.cnt = 0u; a.W = 0.0f; a.Sx = a.Sy = a.Sz = 0.0f; }

struct ShellK {
    float R, R2, offset;
    uint32_t minCount;
};

// One accepted candidate of pass 1.
__host__ __device__ inline void shell_add(ShellAcc& a, float dx, float dy, float dz, float r2, float R2) {
    const float t = R2 - r2;
    const float w = t * t;
    a.cnt += 1u;
    a.W = a.W + w;
    a.Sx = fmaf(w, dx, a.Sx); a.Sy = fmaf(w, dy, a.Sy); a.Sz = fmaf(w, dz, a.Sz);
}
// The record of a target that walked (crest stays 0).
__host__ __device__ inline void shell_finish(const ShellAcc& a, const ShellK& sk, ShellRow& out) {
    const float s2 = dot3(a.Sx, a.Sy, a.Sz, a.Sx, a.Sy, a.Sz);
    const float lim = (sk.offset * sk.R) * a.W;
    const bool in = a.cnt == 0u || a.cnt < sk.minCount || s2 > lim * lim;
    const float len = sqrtf(s2);
    const bool dir = s2 != 0.0f;
    out.normal[0] = dir ? (-a.Sx) / len : 0.0f;
    out.normal[1] = dir ? (-a.Sy) / len : 0.0f;
    out.normal[2] = dir ? (-a.Sz) / len : 0.0f;
    out.offsetRatio = a.W != 0.0f ? len / (sk.R * a.W) : 0.0f;
    out.crest = 0.0f;
    out.count = a.cnt;
    out.flags = (in ? kShellMember : 0u) | (a.cnt == 0u ? kShellIsolated : 0u);
    out.pad = 0u;
}
__host__ __device__ inline void shell_zero(ShellRow& out) {
    out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
    out.offsetRatio = out.crest = 0.0f;
    out.count = out.flags = out.pad = 0u;
}
// One accepted shell candidate of pass 2: (nx, ny, nz) the target's normal, (mx, my, mz) the candidate's.  The term
// (1 - dot(n_i, n_j)) * (1 - sqrt(r2) / R), rounded once to fp32, enters the sum in units of 2^-32, truncated: integer additions, so the
// sum does not depend on the order of the candidates (inside a cell that order is the order of the particle ids).  |term| <= 2 and a
// stencil holds fewer than 2^24 candidates: the sum stays below 2^58.
constexpr float kShellCrestScale = 4294967296.0f;     // 2^32
__host__ __device__ inline long long shell_crest_term(float nx, float ny, float nz, float mx, float my, float mz, float dx, float dy, float dz,
                                                      float r2, float R) {
    if (!(dot3(dx, dy, dz, nx, ny, nz) < 0.0f)) return 0ll;
    const float turn = 1.0f - dot3(nx, ny, nz, mx, my, mz);
    const float close = 1.0f - sqrtf(r2) / R;
    const float term = turn * close;
    if (!(fabsf(term) <= 4.0f)) return 0ll;                                      // (never met with unit normals: keeps the conversion defined)
    return (long long)(term * kShellCrestScale);                                 // (the scaling is exact; the conversion truncates)
}
// The crest of a row from its sum: through double (exact below 2^53, and one correctly rounded conversion on either side beyond).
__host__ __device__ inline float shell_crest_value(long long sum) { return (float)((double)sum * (1.0 / 4294967296.0)); }

// (isolated rows, largest count) of the wave into stats[0], stats[1]: every lane of the wave must arrive.
__device__ __forceinline__ void shell_reduce(bool isolated, uint32_t cnt, unsigned long long* __restrict__ stats) {
    const uint32_t m = wave_max(cnt);
    const unsigned long long ni = (unsigned long long)__popcll(__ballot(isolated));
    if ((threadIdx.x & 63) == 0) {
        if (ni) atomicAdd(stats + 0, ni);
        if (m) atomicMax(stats + 1, (unsigned long long)m);
    }
}

// Pass 1 of a target at P (sorted slot `self`, left out where SKIP): the zero row where it does not walk.
template <bool SKIP>
__device__ __forceinline__ ShellRow shell_row(const SimK& k, const NbK& nb, const ShellK& sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                              const float4* __restrict__ own, bool fluidOnly, const float4& P, uint32_t self, bool walk) {
    ShellRow r;
    shell_zero(r);
    if (walk) {
        ShellAcc a;
        shell_reset(a);
        neighbor_gather<SKIP>(k, nb, pv, cellStart, own, fluidOnly, P, self, [&](float dx, float dy, float dz, float r2) { shell_add(a, dx, dy, dz, r2, nb.R2); });
        shell_finish(a, sk, r);
    }
    return r;
}

// Pass 2 of the shell slot q at P with normal N: the crest sum over its shell candidates (nrmSlot[j].w != 0), in fixed point.
__device__ __forceinline__ long long shell_crest_sum(const SimK& k, const NbK& nb, const ShellK& sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                     const float4* __restrict__ nrmSlot, uint32_t q, const float4& P, const float4& N) {
    long long crest = 0ll;
    const int3 cell = cell_of(k, P.x, P.y, P.z);
    neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
        for (uint32_t j = qs; j < qe; ++j) {
            const float4 M = nrmSlot[j];
            if (M.w == 0.0f || j == q) continue;                              // not in the shell: nothing else is read
            const float4 J = pv[2u * j];
            float dx, dy, dz, r2;
            if (!neighbor_offset(P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2)) continue;
            crest += shell_crest_term(N.x, N.y, N.z, M.x, M.y, M.z, dx, dy, dz, r2, sk.R);
        }
    });
    return crest;
}

template <bool PARTICLES>
__global__ __launch_bounds__(kBlock) void k_shell_gather(SimK k, NbK nb, ShellK sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                         const int32_t* __restrict__ ids, const float4* __restrict__ own,
                                                         const float4* __restrict__ points, size_t rows, ShellRow* __restrict__ out,
                                                         uint32_t* __restrict__ flagRow, float4* __restrict__ nrmSlot, uint32_t* __restrict__ flagSlot,
                                                         unsigned long long* __restrict__ stats) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool fluidOnly = (nb.flags & kShellFluidOnly) != 0;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    size_t row = 0;
    bool walk = false;
    const bool act = query_target<PARTICLES>(pv, ids, points, rows, i, P, row, walk);
    walk = act && sample_finite(P.x, P.y, P.z);                               // (a non-finite particle has an all-zero row here)
    if (PARTICLES && walk && fluidOnly) walk = !slot_ghost(own, (uint32_t)i);
    ShellRow r;
    shell_zero(r);
    if (walk) {                                                               // (shell_row's text, see the file comment)
        ShellAcc a;
        shell_reset(a);
        const uint32_t q = (uint32_t)i;
        const int3 cell = cell_of(k, P.x, P.y, P.z);
        neighbor_rows(k, cellStart, nb.s, nb.n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                if (PARTICLES && j == q) continue;
                const float4 J = pv[2u * j];
                float dx, dy, dz, r2;
                if (!neighbor_offset(P.x, P.y, P.z, J.x, J.y, J.z, nb.R2, dx, dy, dz, r2)) continue;
                if (fluidOnly && slot_ghost(own, j)) continue;
                shell_add(a, dx, dy, dz, r2, nb.R2);
            }
        });
        shell_finish(a, sk, r);
    }
    if (act) {
        const uint32_t in = r.flags & kShellMember;
        float4* o4 = reinterpret_cast<float4*>(out + row);                    // one 32-byte row as two 16-byte stores
        o4[0] = make_float4(r.normal[0], r.normal[1], r.normal[2], r.offsetRatio);
        o4[1] = make_float4(r.crest, bitsf(r.count), bitsf(r.flags), bitsf(r.pad));
        flagRow[row] = in;
        if (PARTICLES) {
            nrmSlot[i] = make_float4(r.normal[0], r.normal[1], r.normal[2], in ? 1.0f : 0.0f);
            flagSlot[i] = in;
        }
    }
    shell_reduce(walk && (r.flags & kShellIsolated), r.count, stats);
}

__global__ __launch_bounds__(kBlock) void k_shell_crest(SimK k, NbK nb, ShellK sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                        const int32_t* __restrict__ ids, const float4* __restrict__ nrmSlot,
                                                        const int32_t* __restrict__ shellSlots, size_t numShell, size_t rows, ShellRow* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= numShell) return;
    const uint32_t q = (uint32_t)shellSlots[t];
    if (q >= nb.n) return;
    const size_t row = (size_t)(uint32_t)ids[q];
    if (row >= rows) return;
    const float4 P = pv[2u * q];
    const float4 N = nrmSlot[q];
    out[row].crest = shell_crest_value(shell_crest_sum(k, nb, sk, pv, cellStart, nrmSlot, q, P, N));
}

// ---- the two passes by slot, for a substep that reads normals and crests itself (the crest births of the diffuse pool) ----
// Nothing by id, no reduction, no host-side count: both launches are sized by n.  A launch is gated by a 64-bit counter (two words) and a
// period, both in device memory: it works when the counter is a multiple of the period and returns at once otherwise, since a captured
// graph has a fixed launch list.
__device__ __forceinline__ bool shell_gate(const uint32_t* __restrict__ counter, const uint32_t* __restrict__ period) {
    const uint32_t p = *period;
    return p != 0u && (((unsigned long long)counter[1] << 32) | counter[0]) % p == 0ull;
}

// Pass 1 by slot (shell_row<true>): writes only the by-slot float4 (normal, 0 outside the shell | 1 member | 2 isolated
// member) and the by-slot 0 / 1 flag word for the scan.
__global__ __launch_bounds__(kBlock) void k_shell_slot_gather(SimK k, NbK nb, ShellK sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                              const float4* __restrict__ own, const uint32_t* __restrict__ counter,
                                                              const uint32_t* __restrict__ period, float4* __restrict__ nrmSlot,
                                                              uint32_t* __restrict__ flagSlot) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nb.n || !shell_gate(counter, period)) return;
    const bool fluidOnly = (nb.flags & kShellFluidOnly) != 0;
    const float4 P = pv[2u * q];
    bool walk = sample_finite(P.x, P.y, P.z);                                 // (a non-finite particle has an all-zero row)
    if (walk && fluidOnly) walk = !slot_ghost(own, q);
    const ShellRow r = shell_row<true>(k, nb, sk, pv, cellStart, own, fluidOnly, P, q, walk);
    const uint32_t in = r.flags & kShellMember;
    nrmSlot[q] = make_float4(r.normal[0], r.normal[1], r.normal[2], in ? ((r.flags & kShellIsolated) ? 2.0f : 1.0f) : 0.0f);
    flagSlot[q] = in;
}

// Pass 2 by slot (shell_crest_sum) over the compacted shell slots.  The launch is sized by n; the number of targets is the word behind
// the scan (numShell, device memory), clamped to n.  One float per slot: lane t clears the slot t where it is no shell member, and writes
// the crest of the t-th shell slot where there is one -- the two sets of slots are disjoint.
__global__ __launch_bounds__(kBlock) void k_shell_slot_crest(SimK k, NbK nb, ShellK sk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                             const float4* __restrict__ nrmSlot, const int32_t* __restrict__ shellSlots,
                                                             const long long* __restrict__ numShell, const uint32_t* __restrict__ counter,
                                                             const uint32_t* __restrict__ period, float* __restrict__ crestSlot) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nb.n || !shell_gate(counter, period)) return;
    if (nrmSlot[t].w == 0.0f) crestSlot[t] = 0.0f;
    const long long total = *numShell;
    if (total <= 0ll || (long long)t >= total) return;                        // (t < nb.n already: the count is clamped to n)
    const uint32_t q = (uint32_t)shellSlots[t];
    if (q >= nb.n) return;
    const float4 P = pv[2u * q];
    const float4 N = nrmSlot[q];
    crestSlot[q] = shell_crest_value(shell_crest_sum(k, nb, sk, pv, cellStart, nrmSlot, q, P, N));
}

}  // namespace sph
