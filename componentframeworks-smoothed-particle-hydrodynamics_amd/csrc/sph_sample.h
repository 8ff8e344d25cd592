// sph_sample.h -- SPH field sampling at probe points and on regular lattices (no reference counterpart).
//
// A probe at x sees exactly the candidates sweep 1 of the SPH pass sees for a particle at x: the members of the
// <= 27 cells around x's cell (BuildGrid's cell formula: (x - gridMin) / cellSize, floorf, clamped to the grid),
// 9 rows in (dz, dy) order, each row one contiguous run of sorted slots, members ascending by id.  Per candidate j,
// t_j = max(h^2 - r^2, 0) with r^2 = dot3(x - x_j):
//   density  = mp6 * sum t_j^3                       (dsum = fmaf(t*t, t, dsum): sweep 1's sum, not clamped)
//   count    = #{ j : r^2 < h^2 }
//   fraction = mp6 * sum invRho_j t_j^3              (Shepard sum: ~1 inside the fluid, 0 outside)
//   vel, P   = sum w_j v_j / sum w_j, w_j = invRho_j t_j^3   (0 where sum w_j = 0)
// so fmaxf(density(x_i), rho0 / 2) at a particle's position is the density the next substep gives it, bit for bit.
// A probe with a non-finite coordinate gives an all-zero record.
//
//   k_sample_points   one probe per thread, the 9 row runs straight from global memory (the bit-level yardstick)
//   k_sample_lattice  implicit points origin + (float)i * spacing (x fastest); a block owns a brick of 8 x 8 x 4 points,
//                     stages the row runs of the brick's cell range +-1 into LDS once (16 bytes per record, 32 when
//                     velocity or pressure is asked for) and walks them from there; a brick whose rows do not fit
//                     walks global memory instead.  Same candidate function, same order, therefore the same bits.
//                     The brick walk hands each point's sample to a sink: this kernel stores it, k_monitor_lattice
//                     (sph_monitor.h) accumulates it.
#pragma once
#include "sph_kernels.h"

namespace sph {

// SPH_FIELD_* of sph_abi.h
constexpr int kFieldDensity = 0, kFieldFraction = 1, kFieldPressure = 2, kFieldSpeed = 3, kFieldAll = 4;

struct SampleAcc {
    float dsum, wsum, vx, vy, vz, p;
    uint32_t cnt;
};

__device__ __forceinline__ void sample_reset(SampleAcc& a) {
    a.dsum = a.wsum = a.vx = a.vy = a.vz = a.p = 0.0f;
    a.cnt = 0u;
}

// The one per-candidate step both kernels share.  J = (x, y, z, 1/rho), JV = (vx, vy, vz, P) of the sorted copy.
template <bool VEL>
__device__ __forceinline__ void sample_candidate(const SimK& k, float px, float py, float pz, const float4& J, const float4& JV, SampleAcc& a) {
    const float dx = px - J.x, dy = py - J.y, dz = pz - J.z;
    const float r2 = dot3(dx, dy, dz, dx, dy, dz);
    const float t = fmaxf(k.h2 - r2, 0.0f);
    a.dsum = fmaf(t * t, t, a.dsum);
    a.cnt += (r2 < k.h2) ? 1u : 0u;
    const float w = ((t * t) * t) * J.w;
    a.wsum += w;
    if (VEL) {
        a.vx = fmaf(w, JV.x, a.vx); a.vy = fmaf(w, JV.y, a.vy); a.vz = fmaf(w, JV.z, a.vz);
        a.p = fmaf(w, JV.w, a.p);
    }
}

struct SampleOut {
    float density, fraction, pressure;
    uint32_t count;
    float vx, vy, vz, pad;
};

__device__ __forceinline__ SampleOut sample_finish(const SimK& k, const SampleAcc& a) {
    SampleOut o;
    o.density = k.mp6 * a.dsum;
    o.fraction = k.mp6 * a.wsum;
    o.count = a.cnt;
    const bool any = a.wsum > 0.0f;
    o.vx = any ? a.vx / a.wsum : 0.0f;
    o.vy = any ? a.vy / a.wsum : 0.0f;
    o.vz = any ? a.vz / a.wsum : 0.0f;
    o.pressure = any ? a.p / a.wsum : 0.0f;
    o.pad = 0.0f;
    return o;
}

// The 9 candidate rows of x's cell, in canonical order: f(row, nz, ny, first slot, end slot).
template <class F>
__device__ __forceinline__ void sample_rows(const SimK& k, const uint32_t* __restrict__ cellStart, int cx, int cy, int cz, F&& f) {
    const int xlo = max(cx - 1, 0), xhi = min(cx + 1, k.gx - 1);
    for (int r = 0; r < 9; ++r) {
        const int nz = cz + r / 3 - 1, ny = cy + r % 3 - 1;
        if (nz < 0 || nz >= k.gz || ny < 0 || ny >= k.gy) continue;
        const int rowBase = (nz * k.gy + ny) * k.gx;
        f(nz, ny, cellStart[rowBase + xlo], cellStart[rowBase + xhi + 1]);
    }
}

template <bool VEL>
__device__ __forceinline__ SampleAcc sample_global(const SimK& k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                   float px, float py, float pz) {
    SampleAcc a;
    sample_reset(a);
    const int3 cell = cell_of(k, px, py, pz);
    sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int, int, uint32_t qs, uint32_t qe) {
        for (uint32_t q = qs; q < qe; ++q) {
            const float4 J = pv[2u * q];
            const float4 JV = VEL ? pv[2u * q + 1u] : J;
            sample_candidate<VEL>(k, px, py, pz, J, JV, a);
        }
    });
    return a;
}

// sample_global's walk with the loads of AHEAD candidates issued together: a lane's walk is a chain of dependent cache misses
// otherwise.  The candidates are accumulated in the same order, so the bits are sample_global's (tracers, monitors).
template <int AHEAD>
__device__ __forceinline__ SampleAcc sample_ahead(const SimK& k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                  float x, float y, float z) {
    SampleAcc a;
    sample_reset(a);
    const int3 cell = cell_of(k, x, y, z);
    sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int, int, uint32_t qs, uint32_t qe) {
        uint32_t q = qs;
        for (; q + (uint32_t)AHEAD <= qe; q += (uint32_t)AHEAD) {
            float4 J[AHEAD], V[AHEAD];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) { J[u] = pv[2u * (q + (uint32_t)u)]; V[u] = pv[2u * (q + (uint32_t)u) + 1u]; }
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) sample_candidate<true>(k, x, y, z, J[u], V[u], a);
        }
        for (; q < qe; ++q) sample_candidate<true>(k, x, y, z, pv[2u * q], pv[2u * q + 1u], a);
    });
    return a;
}

__device__ __forceinline__ void sample_store(void* out, size_t idx, int field, const SampleOut& o) {
    if (field == kFieldAll) {
        float4* d = reinterpret_cast<float4*>(out) + 2 * idx;
        d[0] = make_float4(o.density, o.fraction, o.pressure, bitsf(o.count));
        d[1] = make_float4(o.vx, o.vy, o.vz, 0.0f);
        return;
    }
    float v;
    if (field == kFieldDensity) v = o.density;
    else if (field == kFieldFraction) v = o.fraction;
    else if (field == kFieldPressure) v = o.pressure;
    else v = sqrtf((o.vx * o.vx + o.vy * o.vy) + o.vz * o.vz);
    reinterpret_cast<float*>(out)[idx] = v;
}

// ---- probes: one per thread; points4 = (x, y, z, unused); out = 32-byte SphSample per probe ----
__global__ __launch_bounds__(kBlock) void k_sample_points(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                          const float4* __restrict__ points, void* __restrict__ out, size_t m) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 x = points[i];
    SampleOut o{};
    if (sample_finite(x.x, x.y, x.z)) o = sample_finish(k, sample_global<true>(k, pv, cellStart, x.x, x.y, x.z));
    sample_store(out, i, kFieldAll, o);
}

// ---- lattices ----
constexpr int kBrickX = 8, kBrickY = 8, kBrickZ = 4;                  // 256 points = one block
#ifndef SPH_SAMPLE_STAGE_F4
#define SPH_SAMPLE_STAGE_F4 2048   // 32 KiB of staged records per block (2048 16-byte / 1024 32-byte records): 5 blocks per CU
#endif
constexpr int kStageF4 = SPH_SAMPLE_STAGE_F4;
constexpr int kStageRows = 64;                                         // staged rows at most (one lane of wave 0 each)
constexpr int kSampleStage = 1;                                        // sph_sample_lattice stages bricks (0: the plain walk for every brick)

struct LatticeK {
    float ox, oy, oz, sx, sy, sz;
    int dx, dy, dz;
    int nbx, nby;
    long long nBricks;
    int field;
    int stage;      // 0: every brick walks global memory (the plain kernel)
};

__device__ __forceinline__ float lattice_coord(float o, int i, float s) { return o + (float)i * s; }   // a multiply, then an add (no fma: -ffp-contract=off)

// sink(point index (x fastest), SampleOut): what becomes of a point's sample (k_sample_lattice stores it, a monitor accumulates it).
template <bool VEL, class SINK>
__device__ __forceinline__ void lattice_brick(const SimK& k, const LatticeK& L, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                              SINK&& sink, long long b, float4* st, uint32_t* rowQs, uint32_t* rowOff, int* meta) {
    constexpr int recF4 = VEL ? 2 : 1;
    const int tid = threadIdx.x;
    const int bx = (int)(b % L.nbx), by = (int)((b / L.nbx) % L.nby), bz = (int)(b / ((long long)L.nbx * L.nby));
    const int i = bx * kBrickX + (tid & (kBrickX - 1)), j = by * kBrickY + ((tid / kBrickX) & (kBrickY - 1)), l = bz * kBrickZ + tid / (kBrickX * kBrickY);
    // the brick's cell range: the point -> cell map is monotone per axis, so the corner points bound it
    if (tid < 64) {
        const int lane = tid;
        int staged = 0, cxlo = 0, cxhi = -1, cylo = 0, nyS = 0, czlo = 0, rows = 0;
        if (L.stage) {
            const int i0 = bx * kBrickX, i1 = min(i0 + kBrickX, L.dx) - 1;
            const int j0 = by * kBrickY, j1 = min(j0 + kBrickY, L.dy) - 1;
            const int l0 = bz * kBrickZ, l1 = min(l0 + kBrickZ, L.dz) - 1;
            const float x0 = lattice_coord(L.ox, i0, L.sx), x1 = lattice_coord(L.ox, i1, L.sx);
            const float y0 = lattice_coord(L.oy, j0, L.sy), y1 = lattice_coord(L.oy, j1, L.sy);
            const float z0 = lattice_coord(L.oz, l0, L.sz), z1 = lattice_coord(L.oz, l1, L.sz);
            if (sample_finite(x0, y0, z0) && sample_finite(x1, y1, z1)) {
                cxlo = max(cell_axis(x0, k.gminx, k.cellSize, k.gx) - 1, 0); cxhi = min(cell_axis(x1, k.gminx, k.cellSize, k.gx) + 1, k.gx - 1);
                cylo = max(cell_axis(y0, k.gminy, k.cellSize, k.gy) - 1, 0);
                const int cyhi = min(cell_axis(y1, k.gminy, k.cellSize, k.gy) + 1, k.gy - 1);
                czlo = max(cell_axis(z0, k.gminz, k.cellSize, k.gz) - 1, 0);
                const int czhi = min(cell_axis(z1, k.gminz, k.cellSize, k.gz) + 1, k.gz - 1);
                nyS = cyhi - cylo + 1;
                rows = nyS * (czhi - czlo + 1);
                staged = rows <= kStageRows ? 1 : 0;
            }
        }
        if (staged) {                                                  // wave-uniform
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
            staged = (total * (uint32_t)recF4 <= (uint32_t)kStageF4) ? 1 : 0;
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
            const uint32_t q = rowQs[lo] + (e - rowOff[lo]);
            st[recF4 * e] = pv[2u * q];
            if (VEL) st[recF4 * e + 1] = pv[2u * q + 1u];
        }
    }
    __syncthreads();
    if (i < L.dx && j < L.dy && l < L.dz) {
        const float px = lattice_coord(L.ox, i, L.sx), py = lattice_coord(L.oy, j, L.sy), pz = lattice_coord(L.oz, l, L.sz);
        SampleOut o{};
        if (sample_finite(px, py, pz)) {
            SampleAcc a;
            if (staged) {
                sample_reset(a);
                const int rows = meta[1], cylo = meta[2], nyS = meta[3], czlo = meta[4];
                const int3 cell = cell_of(k, px, py, pz);
                sample_rows(k, cellStart, cell.x, cell.y, cell.z, [&](int nz, int ny, uint32_t qs, uint32_t qe) {
                    const int sr = (nz - czlo) * nyS + (ny - cylo);
                    const bool inRows = ny >= cylo && ny < cylo + nyS && sr >= 0 && sr < rows;
                    const uint32_t base = inRows ? rowOff[sr] : 0u, first = inRows ? rowQs[sr] : 0u, len = inRows ? rowOff[sr + 1] - base : 0u;
                    if (inRows && qs >= first && qe <= first + len) {  // (always, by monotonicity; kept so that LDS is never read outside the rows)
                        for (uint32_t q = qs; q < qe; ++q) {
                            const uint32_t e = base + (q - first);
                            const float4 J = st[recF4 * e];
                            const float4 JV = VEL ? st[recF4 * e + 1] : J;
                            sample_candidate<VEL>(k, px, py, pz, J, JV, a);
                        }
                    } else {
                        for (uint32_t q = qs; q < qe; ++q) {
                            const float4 J = pv[2u * q];
                            const float4 JV = VEL ? pv[2u * q + 1u] : J;
                            sample_candidate<VEL>(k, px, py, pz, J, JV, a);
                        }
                    }
                });
            } else {
                a = sample_global<VEL>(k, pv, cellStart, px, py, pz);
            }
            o = sample_finish(k, a);
        }
        sink(((size_t)l * (size_t)L.dy + (size_t)j) * (size_t)L.dx + (size_t)i, o);
    }
    __syncthreads();                                                   // LDS is reused by the next brick
}

__global__ __launch_bounds__(kBlock) void k_sample_lattice(SimK k, LatticeK L, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                           void* __restrict__ out) {
    __shared__ float4 st[kStageF4];
    __shared__ uint32_t rowQs[kStageRows], rowOff[kStageRows + 1];
    __shared__ int meta[8];
    const bool vel = L.field != kFieldDensity && L.field != kFieldFraction;
    auto store = [&](size_t idx, const SampleOut& o) { sample_store(out, idx, L.field, o); };
    for (long long b = blockIdx.x; b < L.nBricks; b += gridDim.x) {
        if (vel) lattice_brick<true>(k, L, pv, cellStart, store, b, st, rowQs, rowOff, meta);
        else lattice_brick<false>(k, L, pv, cellStart, store, b, st, rowQs, rowOff, meta);
    }
}

}  // namespace sph
