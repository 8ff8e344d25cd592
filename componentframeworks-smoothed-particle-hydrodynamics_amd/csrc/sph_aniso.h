// sph_aniso.h -- anisotropic kernels (Yu & Turk 2013): per particle a smoothed centre and an ellipsoid from the weighted covariance of
// its neighbourhood, and the lattice of the anisotropic fraction summed from those ellipsoids (no reference counterpart; DESIGN.md
// section 3q).
//
// Grid, radius rules, stencil, candidates and the target of a lane are those of sph_query.h (neighbor_stencil, neighbor_rows,
// query_target; the candidate walk is neighbor_gather, the own slot included).  Only positions enter the ellipsoid; 1/rho of the sorted
// copy enters the amplitude.
//
//   aniso_add / aniso_finish / aniso_node_term / aniso_node_value / aniso_coord   __host__ __device__: sph_aniso_host and
//                             sph_aniso_lattice_host run the same functions over HostGrid in the same row order, so the device gives the
//                             twins' bytes.  sqrtf and the divisions are correctly rounded on both sides (hipcc's defaults); every other
//                             operation is rounded on its own (-ffp-contract=off) except the fmaf()s written out below.  WHERE fmaf IS
//                             USED: the sums S_a = fmaf(w, d_a, S_a) and M_ab = fmaf(w * d_a, d_b, M_ab); dot3 (sph_device.h) wherever a
//                             dot product stands; a Jacobi rotation's pairs (x, y) -> (fmaf(-s, y, c * x), fmaf(s, x, c * y)); the
//                             centre fmaf(lambda, m_a, x_a); Q_ab = fmaf(w2 v2a, v2b, fmaf(w1 v1a, v1b, (w0 v0a) v0b)); the rows of
//                             Q r (fmaf(Q_az, r_z, fmaf(Q_ay, r_y, Q_ax * r_x))); and the node's sum fmaf(amplitude, (u * u) * u, acc).
//                             Nothing else is fused.  fminf / fmaxf of the definition are written as selects (aniso_min / aniso_max:
//                             a NaN value gives the bound, the second operand, and so does a tie), so that the sign of a zero is the
//                             same on both sides.
//                             No cbrtf, no trigonometry, no floating-point atomics.
//   k_aniso_gather            one particle per lane in sorted-slot order (neighbor_gather<false>): 16 bytes per candidate, the
//                             eleven sums lane-owned, the Jacobi fully unrolled (p, q compile-time), the 64-byte row as four 16-byte
//                             stores by particle id and the 48-byte slot record as three by sorted slot; (sparse rows, clamped rows,
//                             largest count, largest reach as bits) go to stats with one integer atomic per wave and word.
//   k_aniso_lattice           one node per lane, the 8 x 8 x 4 brick mapping of k_sample_lattice so that a wave's lanes share rows; the
//                             plain walk over global memory: a rejected candidate costs its first float4, an accepted one the other two.
// The range guards (row < rows, j < end <= n) stay so that no load or store can leave its array.
#pragma once
#include <math.h>

#include "sph_query.h"
#include "sph_sample.h"

namespace sph {

constexpr int kAnisoFluidOnly = 1;                                            // SPH_ANISO_FLUID_ONLY of sph_abi.h
constexpr uint32_t kAnisoValid = 1u, kAnisoSparse = 2u, kAnisoClamped = 4u;   // SPH_ANISO_VALID, _SPARSE, _CLAMPED: flags of a row
constexpr int kAnisoSweeps = 5;                                               // cyclic Jacobi sweeps (every off-diagonal is 0 after them)

struct AnisoRow {                                     // SphAniso of sph_abi.h
    float center[3];
    uint32_t count;
    float axis0[3];
    uint32_t flags;
    float axis1[3];
    float reach;
    float axis2[3];
    float amplitude;
};
static_assert(sizeof(AnisoRow) == 64, "SphAniso is 64 bytes");

struct AnisoSlot {                                    // what a lattice node reads of a sorted slot: three float4
    float cx, cy, cz, rho2;
    float qxx, qyy, qzz, qxy;
    float qxz, qyz, amp, pad;
};
static_assert(sizeof(AnisoSlot) == 48, "a slot record is three float4");

struct AnisoAcc {
    uint32_t cnt;
    float W, Sx, Sy, Sz, Mxx, Myy, Mzz, Mxy, Mxz, Myz;
};
__host__ __device__ inline void aniso_reset(AnisoAcc& a) {
    a.cnt = 0u;
    a.W = a.Sx = a.Sy = a.Sz = a.Mxx = a.Myy = a.Mzz = a.Mxy = a.Mxz = a.Myz = 0.0f;
}

struct AnisoK {
    float R2, scale;                                  // scale = 11.0f / R2: C is the identity for a full, uniformly filled neighbourhood
    float support, lambda, maxRatio, maxStretch, sparseScale;
    uint32_t minCount;
};

__host__ __device__ __forceinline__ float aniso_min(float a, float b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ float aniso_max(float a, float b) { return a > b ? a : b; }

// One accepted candidate (the particle's own slot is one: d = 0, w = R2^3).
__host__ __device__ inline void aniso_add(AnisoAcc& a, float dx, float dy, float dz, float r2, float R2) {
    const float t = R2 - r2;
    const float w = (t * t) * t;
    a.cnt += 1u;
    a.W = a.W + w;
    a.Sx = fmaf(w, dx, a.Sx); a.Sy = fmaf(w, dy, a.Sy); a.Sz = fmaf(w, dz, a.Sz);
    const float wx = w * dx, wy = w * dy, wz = w * dz;
    a.Mxx = fmaf(wx, dx, a.Mxx); a.Myy = fmaf(wy, dy, a.Myy); a.Mzz = fmaf(wz, dz, a.Mzz);
    a.Mxy = fmaf(wx, dy, a.Mxy); a.Mxz = fmaf(wx, dz, a.Mxz); a.Myz = fmaf(wy, dz, a.Myz);
}

// A symmetric 3 x 3 matrix (d[k] = a_kk, o[0] = a_01, o[1] = a_02, o[2] = a_12) and the eigenvector columns V[row][column].
struct AnisoEig {
    float d[3], o[3], v[3][3];
};
// The off-diagonal a_pq lives in o[p + q - 1]; the third index is r = 3 - p - q, a_rp in o[r + p - 1], a_rq in o[r + q - 1].
template <int P, int Q>
__host__ __device__ __forceinline__ void aniso_rotate(AnisoEig& m) {
    constexpr int R = 3 - P - Q;
    const float apq = m.o[P + Q - 1];
    if (apq == 0.0f) return;
    const float th = (m.d[Q] - m.d[P]) / (2.0f * apq);
    const float tt = 1.0f / (fabsf(th) + sqrtf(th * th + 1.0f));
    const float t = th < 0.0f ? -tt : tt;
    const float c = 1.0f / sqrtf(t * t + 1.0f);
    const float s = t * c;
    const float h = t * apq;
    m.d[P] = m.d[P] - h;
    m.d[Q] = m.d[Q] + h;
    m.o[P + Q - 1] = 0.0f;
    const float arp = m.o[R + P - 1], arq = m.o[R + Q - 1];
    m.o[R + P - 1] = fmaf(-s, arq, c * arp);
    m.o[R + Q - 1] = fmaf(s, arp, c * arq);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float vp = m.v[k][P], vq = m.v[k][Q];
        m.v[k][P] = fmaf(-s, vq, c * vp);
        m.v[k][Q] = fmaf(s, vp, c * vq);
    }
}
// Exchange (A, B) of the descending sort: strict compare, the columns move with the values.
template <int A, int B>
__host__ __device__ __forceinline__ void aniso_order(AnisoEig& m) {
    if (!(m.d[A] < m.d[B])) return;
    const float t = m.d[A]; m.d[A] = m.d[B]; m.d[B] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float u = m.v[k][A]; m.v[k][A] = m.v[k][B]; m.v[k][B] = u; }
}
// Eigenvalues in d (descending) and eigenvectors in the columns of v: kAnisoSweeps cyclic sweeps over (0,1), (0,2), (1,2).
__host__ __device__ __forceinline__ void aniso_eigen(AnisoEig& m) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m.v[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll
    for (int sweep = 0; sweep < kAnisoSweeps; ++sweep) {
        aniso_rotate<0, 1>(m);
        aniso_rotate<0, 2>(m);
        aniso_rotate<1, 2>(m);
    }
    aniso_order<0, 1>(m);
    aniso_order<1, 2>(m);
    aniso_order<0, 1>(m);
}

__host__ __device__ inline void aniso_zero(AnisoRow& r, AnisoSlot& s) {
    r.center[0] = r.center[1] = r.center[2] = 0.0f;
    r.axis0[0] = r.axis0[1] = r.axis0[2] = r.axis1[0] = r.axis1[1] = r.axis1[2] = r.axis2[0] = r.axis2[1] = r.axis2[2] = 0.0f;
    r.count = r.flags = 0u;
    r.reach = r.amplitude = 0.0f;
    s.cx = s.cy = s.cz = s.rho2 = s.qxx = s.qyy = s.qzz = s.qxy = s.qxz = s.qyz = s.amp = s.pad = 0.0f;
}

// The mean m = S / W and the scaled covariance C of the sums, as the matrix the Jacobi sweeps start from.
__host__ __device__ inline void aniso_covariance(const AnisoAcc& a, const AnisoK& ak, float& mx, float& my, float& mz, AnisoEig& e) {
    mx = a.Sx / a.W; my = a.Sy / a.W; mz = a.Sz / a.W;
    e.d[0] = (a.Mxx / a.W - mx * mx) * ak.scale;
    e.d[1] = (a.Myy / a.W - my * my) * ak.scale;
    e.d[2] = (a.Mzz / a.W - mz * mz) * ak.scale;
    e.o[0] = (a.Mxy / a.W - mx * my) * ak.scale;
    e.o[1] = (a.Mxz / a.W - mx * mz) * ak.scale;
    e.o[2] = (a.Myz / a.W - my * mz) * ak.scale;
}

// The row and the slot record of a particle at (x, y, z) that walked (cnt >= 1: its own slot).
__host__ __device__ inline void aniso_finish(const AnisoAcc& a, const AnisoK& ak, float x, float y, float z, float invRho, AnisoRow& out, AnisoSlot& slot) {
    float mx, my, mz;
    AnisoEig e;
    aniso_covariance(a, ak, mx, my, mz, e);
    aniso_eigen(e);
    float s0 = sqrtf(aniso_max(e.d[0], 0.0f)), s1 = sqrtf(aniso_max(e.d[1], 0.0f)), s2 = sqrtf(aniso_max(e.d[2], 0.0f));
    uint32_t flags = kAnisoValid;
    if (a.cnt < ak.minCount || !(s0 > 0.0f)) {
        flags |= kAnisoSparse;
        s0 = s1 = s2 = ak.sparseScale;
        e.v[0][0] = 1.0f; e.v[0][1] = 0.0f; e.v[0][2] = 0.0f;
        e.v[1][0] = 0.0f; e.v[1][1] = 1.0f; e.v[1][2] = 0.0f;
        e.v[2][0] = 0.0f; e.v[2][1] = 0.0f; e.v[2][2] = 1.0f;
    } else {
        const float c0 = aniso_min(s0, ak.maxStretch);
        const float lo = c0 / ak.maxRatio;
        const float c1 = aniso_min(aniso_max(s1, lo), ak.maxStretch), c2 = aniso_min(aniso_max(s2, lo), ak.maxStretch);
        if (c0 != s0 || c1 != s1 || c2 != s2) flags |= kAnisoClamped;
        s0 = c0; s1 = c1; s2 = c2;
    }
    const float a0 = ak.support * s0, a1 = ak.support * s1, a2 = ak.support * s2;
    const float i0 = 1.0f / a0, i1 = 1.0f / a1, i2 = 1.0f / a2;
    out.center[0] = fmaf(ak.lambda, mx, x); out.center[1] = fmaf(ak.lambda, my, y); out.center[2] = fmaf(ak.lambda, mz, z);
    out.count = a.cnt;
    out.flags = flags;
    out.axis0[0] = a0 * e.v[0][0]; out.axis0[1] = a0 * e.v[1][0]; out.axis0[2] = a0 * e.v[2][0];
    out.axis1[0] = a1 * e.v[0][1]; out.axis1[1] = a1 * e.v[1][1]; out.axis1[2] = a1 * e.v[2][1];
    out.axis2[0] = a2 * e.v[0][2]; out.axis2[1] = a2 * e.v[1][2]; out.axis2[2] = a2 * e.v[2][2];
    const float ox = out.center[0] - x, oy = out.center[1] - y, oz = out.center[2] - z;
    out.reach = a0 + sqrtf(dot3(ox, oy, oz, ox, oy, oz));
    out.amplitude = invRho * ((i0 * i1) * i2);
    const float w0 = i0 * i0, w1 = i1 * i1, w2 = i2 * i2;
    const float u0x = w0 * e.v[0][0], u0y = w0 * e.v[1][0], u0z = w0 * e.v[2][0];
    const float u1x = w1 * e.v[0][1], u1y = w1 * e.v[1][1], u1z = w1 * e.v[2][1];
    const float u2x = w2 * e.v[0][2], u2y = w2 * e.v[1][2], u2z = w2 * e.v[2][2];
    slot.cx = out.center[0]; slot.cy = out.center[1]; slot.cz = out.center[2];
    slot.rho2 = a0 * a0;
    slot.qxx = fmaf(u2x, e.v[0][2], fmaf(u1x, e.v[0][1], u0x * e.v[0][0]));
    slot.qyy = fmaf(u2y, e.v[1][2], fmaf(u1y, e.v[1][1], u0y * e.v[1][0]));
    slot.qzz = fmaf(u2z, e.v[2][2], fmaf(u1z, e.v[2][1], u0z * e.v[2][0]));
    slot.qxy = fmaf(u2x, e.v[1][2], fmaf(u1x, e.v[1][1], u0x * e.v[1][0]));
    slot.qxz = fmaf(u2x, e.v[2][2], fmaf(u1x, e.v[2][1], u0x * e.v[2][0]));
    slot.qyz = fmaf(u2y, e.v[2][2], fmaf(u1y, e.v[2][1], u0y * e.v[2][0]));
    slot.amp = out.amplitude;
    slot.pad = 0.0f;
}

// A lattice coordinate: a multiply, then an add (lattice_coord of sph_sample.h, on both sides).
__host__ __device__ __forceinline__ float aniso_coord(float o, int i, float s) { return o + (float)i * s; }

// The first test of a candidate at a node: r = x - centre_j, inside the sphere of the longest semi-axis?  Part of the definition.
__host__ __device__ __forceinline__ bool aniso_node_near(float px, float py, float pz, float cx, float cy, float cz, float rho2, float& rx, float& ry, float& rz) {
    rx = px - cx; ry = py - cy; rz = pz - cz;
    return dot3(rx, ry, rz, rx, ry, rz) < rho2;
}
// One near candidate: acc = fmaf(amplitude, max(1 - r'Qr, 0)^3, acc).
__host__ __device__ __forceinline__ float aniso_node_term(float rx, float ry, float rz, float qxx, float qyy, float qzz, float qxy, float qxz, float qyz, float amp,
                                                          float acc) {
    const float tx = fmaf(qxz, rz, fmaf(qxy, ry, qxx * rx));
    const float ty = fmaf(qyz, rz, fmaf(qyy, ry, qxy * rx));
    const float tz = fmaf(qzz, rz, fmaf(qyz, ry, qxz * rx));
    const float q2 = dot3(rx, ry, rz, tx, ty, tz);
    const float u = aniso_max(1.0f - q2, 0.0f);
    return fmaf(amp, (u * u) * u, acc);
}
constexpr float kAnisoPoly = 1.5666815f;              // 315 / (64 pi)
__host__ __device__ __forceinline__ float aniso_node_value(float mass, float acc) { return (mass * kAnisoPoly) * acc; }

// (sparse rows, clamped rows, largest count, largest reach as bits) of the wave into stats[0 .. 4): every lane of the wave must arrive.
// Floats >= 0 order as their bits, so the largest reach is an integer maximum.
__device__ __forceinline__ void aniso_reduce(bool sparse, bool clamped, uint32_t cnt, float reach, unsigned long long* __restrict__ stats) {
    const uint32_t m = wave_max(cnt), rb = wave_max(fbits(reach));
    const unsigned long long ns = (unsigned long long)__popcll(__ballot(sparse)), nc = (unsigned long long)__popcll(__ballot(clamped));
    if ((threadIdx.x & 63) == 0) {
        if (ns) atomicAdd(stats + 0, ns);
        if (nc) atomicAdd(stats + 1, nc);
        if (m) atomicMax(stats + 2, (unsigned long long)m);
        if (rb) atomicMax(stats + 3, (unsigned long long)rb);
    }
}

__global__ __launch_bounds__(kBlock) void k_aniso_gather(SimK k, NbK nb, AnisoK ak, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                         const int32_t* __restrict__ ids, const float4* __restrict__ own, size_t rows,
                                                         AnisoRow* __restrict__ out, float4* __restrict__ slots, unsigned long long* __restrict__ stats) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool fluidOnly = (nb.flags & kAnisoFluidOnly) != 0;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    size_t row = 0;
    bool walk = false;
    const bool act = query_target<true>(pv, ids, nullptr, rows, i, P, row, walk);
    walk = act && sample_finite(P.x, P.y, P.z);                               // (a non-finite particle has an all-zero row)
    if (walk && fluidOnly) walk = !slot_ghost(own, (uint32_t)i);
    AnisoRow r;
    AnisoSlot s;
    aniso_zero(r, s);
    if (walk) {
        AnisoAcc a;
        aniso_reset(a);
        neighbor_gather<false>(k, nb, pv, cellStart, own, fluidOnly, P, 0u, [&](float dx, float dy, float dz, float r2) { aniso_add(a, dx, dy, dz, r2, nb.R2); });
        if (a.cnt) aniso_finish(a, ak, P.x, P.y, P.z, P.w, r, s);                // (always: the particle's own slot is a candidate)
    }
    if (act) {
        float4* o4 = reinterpret_cast<float4*>(out + row);                    // one 64-byte row as four 16-byte stores
        o4[0] = make_float4(r.center[0], r.center[1], r.center[2], bitsf(r.count));
        o4[1] = make_float4(r.axis0[0], r.axis0[1], r.axis0[2], bitsf(r.flags));
        o4[2] = make_float4(r.axis1[0], r.axis1[1], r.axis1[2], r.reach);
        o4[3] = make_float4(r.axis2[0], r.axis2[1], r.axis2[2], r.amplitude);
        float4* s4 = slots + 3u * i;                                          // the slot record as three
        s4[0] = make_float4(s.cx, s.cy, s.cz, s.rho2);
        s4[1] = make_float4(s.qxx, s.qyy, s.qzz, s.qxy);
        s4[2] = make_float4(s.qxz, s.qyz, s.amp, 0.0f);
    }
    aniso_reduce((r.flags & kAnisoSparse) != 0u, (r.flags & kAnisoClamped) != 0u, r.count, r.reach, stats);
}

// L: the lattice (LatticeK of sph_sample.h; field and stage are not read).  s: reachStencil.  slots: 3 float4 per sorted slot.
__global__ __launch_bounds__(kBlock) void k_aniso_lattice(SimK k, LatticeK L, int s, uint32_t n, float mass, const float4* __restrict__ slots,
                                                          const uint32_t* __restrict__ cellStart, float* __restrict__ out) {
    const int tid = threadIdx.x;
    for (long long b = blockIdx.x; b < L.nBricks; b += gridDim.x) {
        const int bx = (int)(b % L.nbx), by = (int)((b / L.nbx) % L.nby), bz = (int)(b / ((long long)L.nbx * L.nby));
        const int i = bx * kBrickX + (tid & (kBrickX - 1)), j = by * kBrickY + ((tid / kBrickX) & (kBrickY - 1)), l = bz * kBrickZ + tid / (kBrickX * kBrickY);
        if (i >= L.dx || j >= L.dy || l >= L.dz) continue;
        const float px = aniso_coord(L.ox, i, L.sx), py = aniso_coord(L.oy, j, L.sy), pz = aniso_coord(L.oz, l, L.sz);
        float acc = 0.0f;
        const bool finite = sample_finite(px, py, pz);                        // (a node with a non-finite coordinate gets 0)
        if (finite) {
            const int3 cell = cell_of(k, px, py, pz);
            neighbor_rows(k, cellStart, s, n, cell.x, cell.y, cell.z, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t q = qs; q < qe; ++q) {
                    const float4 A = slots[3u * (size_t)q];
                    float rx, ry, rz;
                    if (!aniso_node_near(px, py, pz, A.x, A.y, A.z, A.w, rx, ry, rz)) continue;
                    const float4 B = slots[3u * (size_t)q + 1u], C = slots[3u * (size_t)q + 2u];
                    acc = aniso_node_term(rx, ry, rz, B.x, B.y, B.z, B.w, C.x, C.y, C.z, acc);
                }
            });
        }
        out[((size_t)l * (size_t)L.dy + (size_t)j) * (size_t)L.dx + (size_t)i] = finite ? aniso_node_value(mass, acc) : 0.0f;
    }
}

}  // namespace sph
