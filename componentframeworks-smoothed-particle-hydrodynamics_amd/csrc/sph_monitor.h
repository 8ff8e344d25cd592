// sph_monitor.h -- field monitors: fixed probes and lattices averaged inside the substep (no reference counterpart).
//
// A monitor is a fixed set of M points, an explicit list or the lattice origin + (float)i * spacing (x fastest).  Every `every`-th
// non-paused substep ("acting") takes, behind that substep's grid build, the SphSample sph_sample_points would return for each point on
// the state the substep starts from -- sample_rows / sample_candidate / sample_finish of sph_sample.h themselves, same candidate
// order, therefore the same bits -- and adds it to the point's own row of running fp64 sums.  No atomics: a row depends on nothing but
// the sequence of its samples.  Every update is sum = sum + (double)x or sum = sum + (double)a * (double)b; the product of two fp32
// values is exact in fp64, so a fused and an unfused multiply-add give the same bits and the host twin gives the device's bytes.
// A ring keeps the raw samples of the points 0 .. ringPoints-1 with the fp64 time of the entry state.
//
// Everything a captured graph would otherwise bake in lives in device memory (MonitorTab): every, stride, the ring geometry, the
// counters, wetFraction and a lattice's origin and spacing.  A non-acting substep is a launch that reads one word and returns.
//
//   k_monitor_points   one point per lane in a processing order sorted by the point's cell at set time (speed only: a row is read and
//                      written at its caller-order index), candidate loads kMonitorAhead at a time (sample_ahead)
//   k_monitor_lattice  the brick walk of k_sample_lattice (lattice_brick with an accumulating sink): 8 x 8 x 4 points per block, the
//                      rows of the brick's cell range +-1 staged into LDS once, the global-memory walk when they do not fit
//   k_monitor_tick     one thread behind the step: the ring row's time, then c, a, the time and what the next substep does
//   k_monitor_field    the derived volume, one point per thread
#pragma once
#include "sph_sample.h"

namespace sph {

constexpr int kMonitorMax = 4;                       // SPH_MAX_MONITORS
constexpr uint32_t kMonitorNoRow = 0xFFFFFFFFu;
constexpr int kMonitorAhead = 4;                     // candidates whose records are in flight before the first is accumulated
// SPH_MONITOR_* fields of sph_abi.h
constexpr int kMonWetShare = 0, kMonMeanFraction = 1, kMonVarFraction = 2, kMonMeanDensity = 3, kMonMeanPressure = 4, kMonVarPressure = 5,
              kMonMeanVelX = 6, kMonMeanVelY = 7, kMonMeanVelZ = 8, kMonTke = 9, kMonFields = 10;

struct MonitorRow {                                  // SphMonitorRow of sph_abi.h: 128 bytes, one cache line
    unsigned long long samples, wet;
    double sumFraction, sumFraction2, sumDensity;    // over all samples
    double sumPressure, sumPressure2;                // over wet samples
    double sumVel[3];                                // over wet samples
    double sumVelVel[6];                             // xx, yy, zz, xy, xz, yz; wet
};
static_assert(sizeof(MonitorRow) == 128, "MonitorRow is one 128-byte line");

struct MonitorTab {                                  // device memory; the host keeps what it uploaded last
    unsigned long long c;                            // non-paused substeps seen since set / reset
    unsigned long long a;                            // acting substeps among them
    double time;                                     // sum of their dt
    uint32_t every, stride, history, ringPoints;
    float wetFraction;
    uint32_t act;                                    // the substep that runs next acts (c % every == 0)
    uint32_t row;                                    // and writes this ring row, or kMonitorNoRow
    uint32_t pad;
    LatticeK L;                                      // lattice monitors: the brick constants (field and stage as the sampler's)
};

// The rule: substep number c (0-based) acts iff c % every == 0; the acting substep number a (0-based) writes ring row
// (a / stride) % history iff history > 0 && a % stride == 0.
__host__ __device__ inline bool monitor_acts(unsigned long long c, uint32_t every) { return every == 0u || c % every == 0ull; }
__host__ __device__ inline uint32_t monitor_row_of(unsigned long long a, uint32_t history, uint32_t stride) {
    if (history == 0u || stride == 0u || a % stride != 0ull) return kMonitorNoRow;
    return (uint32_t)((a / stride) % history);
}
// One substep of the counters (k_monitor_tick and the host's schedule twin): returns the ring row the substep wrote, or none.
__host__ __device__ inline uint32_t monitor_tick(MonitorTab& t, double dt, bool* acted) {
    uint32_t wrote = kMonitorNoRow;
    *acted = t.act != 0u;
    if (t.act) { wrote = t.row; t.a += 1ull; }
    t.c += 1ull;
    t.time = t.time + dt;
    t.act = monitor_acts(t.c, t.every) ? 1u : 0u;
    t.row = monitor_row_of(t.a, t.history, t.stride);
    return wrote;
}

// One sample into one row.  A sample with a non-finite field is skipped whole (false: the row is unchanged).
__host__ __device__ inline bool monitor_update(MonitorRow& r, float density, float fraction, float pressure, float vx, float vy, float vz, float wetFraction) {
    if (!(float_finite(density) && float_finite(fraction) && float_finite(pressure) && float_finite(vx) && float_finite(vy) && float_finite(vz))) return false;
    const double f = (double)fraction;
    r.samples += 1ull;
    r.sumFraction = r.sumFraction + f;
    r.sumFraction2 = r.sumFraction2 + f * f;
    r.sumDensity = r.sumDensity + (double)density;
    if (fraction >= wetFraction) {
        const double p = (double)pressure, x = (double)vx, y = (double)vy, z = (double)vz;
        r.wet += 1ull;
        r.sumPressure = r.sumPressure + p;
        r.sumPressure2 = r.sumPressure2 + p * p;
        r.sumVel[0] = r.sumVel[0] + x; r.sumVel[1] = r.sumVel[1] + y; r.sumVel[2] = r.sumVel[2] + z;
        r.sumVelVel[0] = r.sumVelVel[0] + x * x; r.sumVelVel[1] = r.sumVelVel[1] + y * y; r.sumVelVel[2] = r.sumVelVel[2] + z * z;
        r.sumVelVel[3] = r.sumVelVel[3] + x * y; r.sumVelVel[4] = r.sumVelVel[4] + x * z; r.sumVelVel[5] = r.sumVelVel[5] + y * z;
    }
    return true;
}

// The derived fields: every operation in fp64 and rounded on its own (-ffp-contract=off), one rounding to fp32 at the end; 0 where
// the dividing count is 0.  No square root.
__host__ __device__ inline double monitor_mean(double sum, unsigned long long n) { return n ? sum / (double)n : 0.0; }
__host__ __device__ inline double monitor_var(double sum2, double sum, unsigned long long n) {
    if (!n) return 0.0;
    const double mean = sum / (double)n, second = sum2 / (double)n, sq = mean * mean;
    return second - sq;
}
__host__ __device__ inline float monitor_field_value(const MonitorRow& r, int field) {
    double v = 0.0;
    switch (field) {
    case kMonWetShare: v = monitor_mean((double)r.wet, r.samples); break;
    case kMonMeanFraction: v = monitor_mean(r.sumFraction, r.samples); break;
    case kMonVarFraction: v = monitor_var(r.sumFraction2, r.sumFraction, r.samples); break;
    case kMonMeanDensity: v = monitor_mean(r.sumDensity, r.samples); break;
    case kMonMeanPressure: v = monitor_mean(r.sumPressure, r.wet); break;
    case kMonVarPressure: v = monitor_var(r.sumPressure2, r.sumPressure, r.wet); break;
    case kMonMeanVelX: v = monitor_mean(r.sumVel[0], r.wet); break;
    case kMonMeanVelY: v = monitor_mean(r.sumVel[1], r.wet); break;
    case kMonMeanVelZ: v = monitor_mean(r.sumVel[2], r.wet); break;
    case kMonTke: {
        const double xx = monitor_var(r.sumVelVel[0], r.sumVel[0], r.wet), yy = monitor_var(r.sumVelVel[1], r.sumVel[1], r.wet),
                     zz = monitor_var(r.sumVelVel[2], r.sumVel[2], r.wet);
        const double s = (xx + yy) + zz;
        v = 0.5 * s;
        break;
    }
    default: break;
    }
    return (float)v;
}

// What becomes of point i's sample in an acting substep: the ring (points below ringPoints), then the read-modify-write of the
// point's own 128-byte row as eight 16-byte accesses.
__device__ __forceinline__ void monitor_sink(const MonitorTab* __restrict__ tab, MonitorRow* __restrict__ rows, float4* __restrict__ ring, size_t i,
                                             const SampleOut& o) {
    const uint32_t row = tab->row, rp = tab->ringPoints;
    if (row != kMonitorNoRow && row < tab->history && i < (size_t)rp) {
        float4* d = ring + 2u * ((size_t)row * rp + i);
        d[0] = make_float4(o.density, o.fraction, o.pressure, bitsf(o.count));
        d[1] = make_float4(o.vx, o.vy, o.vz, 0.0f);
    }
    union { MonitorRow r; ulonglong2 w[8]; } u;
    ulonglong2* line = reinterpret_cast<ulonglong2*>(rows + i);
#pragma unroll
    for (int q = 0; q < 8; ++q) u.w[q] = line[q];
    if (!monitor_update(u.r, o.density, o.fraction, o.pressure, o.vx, o.vy, o.vz, tab->wetFraction)) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) line[q] = u.w[q];
}

__global__ __launch_bounds__(kBlock) void k_monitor_points(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                           const MonitorTab* __restrict__ tab, const float4* __restrict__ points,
                                                           const uint32_t* __restrict__ perm, MonitorRow* __restrict__ rows, float4* __restrict__ ring, uint32_t m) {
    if (!tab->act) return;                                             // (the idle launch of a non-acting substep)
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = perm[t];
    if (i >= m) return;                                                // (never: perm[] is a permutation of [0, m))
    const float4 x = points[i];
    SampleOut o{};                                                     // (a non-finite point: the sampler's all-zero record, a dry sample)
    if (sample_finite(x.x, x.y, x.z)) o = sample_finish(k, sample_ahead<kMonitorAhead>(k, pv, cellStart, x.x, x.y, x.z));
    monitor_sink(tab, rows, ring, (size_t)i, o);
}

__global__ __launch_bounds__(kBlock) void k_monitor_lattice(SimK k, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                            const MonitorTab* __restrict__ tab, MonitorRow* __restrict__ rows, float4* __restrict__ ring) {
    __shared__ float4 st[kStageF4];
    __shared__ uint32_t rowQs[kStageRows], rowOff[kStageRows + 1];
    __shared__ int meta[8];
    if (!tab->act) return;                                             // (block-uniform, before the first barrier)
    const LatticeK L = tab->L;
    auto sink = [&](size_t idx, const SampleOut& o) { monitor_sink(tab, rows, ring, idx, o); };
    for (long long b = blockIdx.x; b < L.nBricks; b += gridDim.x) lattice_brick<true>(k, L, pv, cellStart, sink, b, st, rowQs, rowOff, meta);
}

__global__ void k_monitor_tick(MonitorTab* __restrict__ tab, double* __restrict__ ringTimes, float dt) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    MonitorTab t = *tab;
    const double entry = t.time;
    bool acted;
    const uint32_t wrote = monitor_tick(t, (double)dt, &acted);
    if (wrote != kMonitorNoRow && wrote < t.history) ringTimes[wrote] = entry;
    tab->c = t.c; tab->a = t.a; tab->time = t.time; tab->act = t.act; tab->row = t.row;
}

__global__ __launch_bounds__(kBlock) void k_monitor_field(const MonitorRow* __restrict__ rows, int field, float* __restrict__ out, size_t m) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    out[i] = monitor_field_value(rows[i], field);
}
}  // namespace sph
