// sph_volume.h -- bodies shaped by a lattice of signed distances, and the mesh -> signed distance build (no reference counterpart;
// DESIGN.md section 3f).
//
// A volume is a lattice of fp32 signed distances (negative inside the solid, x fastest) centred on a body: local coordinate of point i on
// axis a is (float)i * spacing_a - half_a.  vol_sample is the trilinear interpolant and the gradient of the same interpolant, vol_project
// the two-step projection of a point inside the solid onto the zero level set; both are __host__ __device__ and are what k_obstacles_vol
// (sph_obstacle.h) and sph_volume_sample_host / sph_obstacles_apply_host_volumes run.  -ffp-contract=off: the only fused operations are
// the explicit fmaf() of dot3 (sph_device.h).
//
//   k_mesh_distance   all pairs (lattice point, triangle), tiled like an n-body kernel: a lane owns one lattice point, a block stages
//                     kMeshChunk triangles with their edges into LDS (one triangle per thread, once per chunk) and every lane reads the
//                     same triangle at the same time (LDS broadcast).  Per point: min of the squared distances (closest point on triangle
//                     by the region walk of Ericson 5.1.5) and the fp64 sum of the fp32 solid-angle terms atan2f(det, den) of Van Oosterom
//                     and Strackee.  gridDim.y splits the triangles; every split writes its partial pair.
//   k_mesh_merge      per point: the min of the partial minima (exact: min is associative and commutative), the partial sums added in split
//                     order, w = sum / (2 pi), the result -sqrtf(min) where w >= 0.5 and +sqrtf(min) elsewhere.
// Triangles are counter-clockwise seen from outside (what the mesher of sph_surface.h emits).  A closed mesh wound the other way has
// w = -1 inside and is therefore OUTSIDE everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "sph_device.h"   // dot3, float_finite

namespace sph {

constexpr int kVolMax = 16;                  // SPH_MAX_VOLUMES
constexpr int kVolBodies = 16;               // rows of the binding table (SPH_MAX_OBSTACLES)
constexpr int kMeshBlock = 256;              // threads (= lattice points) per block of k_mesh_distance
constexpr int kMeshChunk = kMeshBlock;       // triangles staged per chunk: one per thread

// One volume slot as the kernels see it (64 bytes).  half and inv are computed once on the host (vol_make).
struct VolRec {
    const float* values;
    int32_t dims[3];
    float half[3];
    float inv[3];
    float spacing[3];
    int32_t pad[2];
};
static_assert(sizeof(VolRec) == 64, "VolRec must be 64 bytes");

// The device table: the slots and, per body, the slot it is bound to (-1: none).
struct VolTable {
    VolRec vol[kVolMax];
    int32_t bind[kVolBodies];
};

__host__ __device__ inline float vol_lerp(float a, float b, float f) { return a + f * (b - a); }   // subtract, multiply, add

// half_a = (0.5f (float)(dims_a - 1)) spacing_a, inv_a = 1.0f / spacing_a.
inline void vol_make(const float* values, const int dims[3], const float spacing[3], VolRec& v) {
    memset(&v, 0, sizeof(v));
    v.values = values;
    for (int a = 0; a < 3; ++a) {
        v.dims[a] = dims[a];
        v.spacing[a] = spacing[a];
        v.half[a] = (0.5f * (float)(dims[a] - 1)) * spacing[a];
        v.inv[a] = 1.0f / spacing[a];
    }
}

// The trilinear interpolant at the local point l and the gradient of the same interpolant (already divided by the spacing).  Lattice
// coordinate g_a = (l_a + half_a) inv_a; outside [0, dims_a - 1] (a NaN is outside) the result is false, or, with clamp, g_a is clamped
// into the extent first (a NaN becomes 0).  Cell i_a = min((int)floorf(g_a), dims_a - 2), f_a = g_a - (float)i_a; lerps in x, then y, then z.
__host__ __device__ inline bool vol_sample(const VolRec& v, float lx, float ly, float lz, bool clamp, float& phi, float (&g)[3]) {
    float gx = (lx + v.half[0]) * v.inv[0], gy = (ly + v.half[1]) * v.inv[1], gz = (lz + v.half[2]) * v.inv[2];
    const float ex = (float)(v.dims[0] - 1), ey = (float)(v.dims[1] - 1), ez = (float)(v.dims[2] - 1);
    if (clamp) {
        gx = fminf(fmaxf(gx, 0.0f), ex); gy = fminf(fmaxf(gy, 0.0f), ey); gz = fminf(fmaxf(gz, 0.0f), ez);
    } else if (!(gx >= 0.0f && gx <= ex && gy >= 0.0f && gy <= ey && gz >= 0.0f && gz <= ez)) {
        return false;
    }
    int ix = (int)floorf(gx), iy = (int)floorf(gy), iz = (int)floorf(gz);
    ix = ix < v.dims[0] - 2 ? ix : v.dims[0] - 2; iy = iy < v.dims[1] - 2 ? iy : v.dims[1] - 2; iz = iz < v.dims[2] - 2 ? iz : v.dims[2] - 2;
    const float fx = gx - (float)ix, fy = gy - (float)iy, fz = gz - (float)iz;
    const size_t nx = (size_t)v.dims[0], nxy = nx * (size_t)v.dims[1];
    const float* p = v.values + ((size_t)iz * nxy + (size_t)iy * nx + (size_t)ix);
    const float c000 = p[0], c100 = p[1], c010 = p[nx], c110 = p[nx + 1];
    const float c001 = p[nxy], c101 = p[nxy + 1], c011 = p[nxy + nx], c111 = p[nxy + nx + 1];
    phi = vol_lerp(vol_lerp(vol_lerp(c000, c100, fx), vol_lerp(c010, c110, fx), fy),
                   vol_lerp(vol_lerp(c001, c101, fx), vol_lerp(c011, c111, fx), fy), fz);
    const float Gx = vol_lerp(vol_lerp(c100 - c000, c110 - c010, fy), vol_lerp(c101 - c001, c111 - c011, fy), fz);   // x-differences: y, then z
    const float Gy = vol_lerp(vol_lerp(c010 - c000, c110 - c100, fx), vol_lerp(c011 - c001, c111 - c101, fx), fz);   // y-differences: x, then z
    const float Gz = vol_lerp(vol_lerp(c001 - c000, c101 - c100, fx), vol_lerp(c011 - c010, c111 - c110, fx), fy);   // z-differences: x, then y
    g[0] = Gx * v.inv[0]; g[1] = Gy * v.inv[1]; g[2] = Gz * v.inv[2];
    return true;
}

// A local point l (already strictly inside the body's box) against the lattice.  0: no hit (outside the extent, phi >= 0 or NaN, or a
// result that is not finite).  1: o is l after two steps o <- o - phi(o) m(o), m = g / |g|, the second evaluation at the lattice point
// clamped into the extent, and m the unit gradient of the second evaluation.  2: a gradient of length 0 or not finite: the box decides.
__host__ __device__ inline int vol_project(const VolRec& v, float lx, float ly, float lz, float& ox, float& oy, float& oz, float& mx, float& my,
                                           float& mz) {
    float phi, g[3];
    if (!vol_sample(v, lx, ly, lz, false, phi, g)) return 0;
    if (!(phi < 0.0f)) return 0;
    float len = sqrtf(dot3(g[0], g[1], g[2], g[0], g[1], g[2]));
    if (len == 0.0f || !float_finite(len)) return 2;
    const float ax = g[0] / len, ay = g[1] / len, az = g[2] / len;
    const float px = lx - phi * ax, py = ly - phi * ay, pz = lz - phi * az;
    vol_sample(v, px, py, pz, true, phi, g);
    len = sqrtf(dot3(g[0], g[1], g[2], g[0], g[1], g[2]));
    if (len == 0.0f || !float_finite(len)) return 2;
    const float bx = g[0] / len, by = g[1] / len, bz = g[2] / len;
    const float qx = px - phi * bx, qy = py - phi * by, qz = pz - phi * bz;
    if (!float_finite(qx) || !float_finite(qy) || !float_finite(qz)) return 0;
    ox = qx; oy = qy; oz = qz; mx = bx; my = by; mz = bz;
    return 1;
}

// ---- mesh -> signed distance --------------------------------------------------------------------
// One staged triangle: its vertices and the edges ab = b - a, ac = c - a, bc = c - b (80 bytes, so that a lane reads it in 16-byte pieces).
struct alignas(16) MeshTri {
    float a[3], b[3], c[3], ab[3], ac[3], bc[3];
    float pad[2];
};
static_assert(sizeof(MeshTri) == 80, "MeshTri must be 80 bytes");

struct MeshLattice {
    float ox, oy, oz, sx, sy, sz;
    int nx, ny, nz;
    long long total;
};

__host__ __device__ inline void mesh_tri_setup(const float* __restrict__ verts, const uint32_t* __restrict__ tri, MeshTri& T) {
    const float* A = verts + 3 * (size_t)tri[0];
    const float* B = verts + 3 * (size_t)tri[1];
    const float* Cc = verts + 3 * (size_t)tri[2];
    for (int i = 0; i < 3; ++i) {
        T.a[i] = A[i]; T.b[i] = B[i]; T.c[i] = Cc[i];
        T.ab[i] = B[i] - A[i]; T.ac[i] = Cc[i] - A[i]; T.bc[i] = Cc[i] - B[i];
    }
    T.pad[0] = T.pad[1] = 0.0f;
}

// Squared distance from p to the triangle: the closest point q by the region walk (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc,
// face, in this order), then dot3(p - q, p - q).  Every operation but the fmaf of dot3 is rounded on its own; the divisions are IEEE.
__host__ __device__ inline float mesh_tri_d2(const MeshTri& T, float px, float py, float pz) {
    const float apx = px - T.a[0], apy = py - T.a[1], apz = pz - T.a[2];
    const float d1 = dot3(T.ab[0], T.ab[1], T.ab[2], apx, apy, apz);
    const float d2 = dot3(T.ac[0], T.ac[1], T.ac[2], apx, apy, apz);
    float qx, qy, qz;
    do {
        if (d1 <= 0.0f && d2 <= 0.0f) { qx = T.a[0]; qy = T.a[1]; qz = T.a[2]; break; }
        const float bpx = px - T.b[0], bpy = py - T.b[1], bpz = pz - T.b[2];
        const float d3 = dot3(T.ab[0], T.ab[1], T.ab[2], bpx, bpy, bpz);
        const float d4 = dot3(T.ac[0], T.ac[1], T.ac[2], bpx, bpy, bpz);
        if (d3 >= 0.0f && d4 <= d3) { qx = T.b[0]; qy = T.b[1]; qz = T.b[2]; break; }
        const float vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
            const float t = d1 / (d1 - d3);
            qx = T.a[0] + t * T.ab[0]; qy = T.a[1] + t * T.ab[1]; qz = T.a[2] + t * T.ab[2];
            break;
        }
        const float cpx = px - T.c[0], cpy = py - T.c[1], cpz = pz - T.c[2];
        const float d5 = dot3(T.ab[0], T.ab[1], T.ab[2], cpx, cpy, cpz);
        const float d6 = dot3(T.ac[0], T.ac[1], T.ac[2], cpx, cpy, cpz);
        if (d6 >= 0.0f && d5 <= d6) { qx = T.c[0]; qy = T.c[1]; qz = T.c[2]; break; }
        const float vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
            const float t = d2 / (d2 - d6);
            qx = T.a[0] + t * T.ac[0]; qy = T.a[1] + t * T.ac[1]; qz = T.a[2] + t * T.ac[2];
            break;
        }
        const float va = d3 * d6 - d5 * d4;
        const float e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
            const float t = e43 / (e43 + e56);
            qx = T.b[0] + t * T.bc[0]; qy = T.b[1] + t * T.bc[1]; qz = T.b[2] + t * T.bc[2];
            break;
        }
        const float s = (va + vb) + vc;
        const float v = vb / s, w = vc / s;
        qx = (T.a[0] + T.ab[0] * v) + T.ac[0] * w; qy = (T.a[1] + T.ab[1] * v) + T.ac[1] * w; qz = (T.a[2] + T.ab[2] * v) + T.ac[2] * w;
    } while (false);
    const float ex = px - qx, ey = py - qy, ez = pz - qz;
    return dot3(ex, ey, ez, ex, ey, ez);
}

// Half the solid angle of the triangle seen from p (Van Oosterom and Strackee): atan2f(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|).
// The winding number is the sum of these over the mesh divided by 2 pi.  (Its bits are not part of the contract, the threshold is.)
__host__ __device__ inline float mesh_tri_angle(const MeshTri& T, float px, float py, float pz) {
    const float ax = T.a[0] - px, ay = T.a[1] - py, az = T.a[2] - pz;
    const float bx = T.b[0] - px, by = T.b[1] - py, bz = T.b[2] - pz;
    const float cx = T.c[0] - px, cy = T.c[1] - py, cz = T.c[2] - pz;
    const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)), lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
    const float det = dot3(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
    const float den = (((la * lb) * lc + dot3(ax, ay, az, bx, by, bz) * lc) + dot3(bx, by, bz, cx, cy, cz) * la) + dot3(cx, cy, cz, ax, ay, az) * lb;
    return atan2f(det, den);
}

__host__ __device__ inline float mesh_signed(float best, double angles) {
    const double w = angles * 0.15915494309189535;                   // 1 / (2 pi)
    const float d = sqrtf(best);
    return w >= 0.5 ? -d : d;
}

// Block (x, y): lattice points x kMeshBlock .. + kMeshBlock - 1 against triangles [y per, min(nt, (y + 1) per)).
__global__ __launch_bounds__(kMeshBlock) void k_mesh_distance(const float* __restrict__ verts, const uint32_t* __restrict__ tris, int nt, int per,
                                                              MeshLattice L, float* __restrict__ d2part, double* __restrict__ wpart) {
    __shared__ MeshTri st[kMeshChunk];
    const long long p = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
    const bool valid = p < L.total;
    const long long pc = valid ? p : 0;
    const int i = (int)(pc % L.nx), j = (int)((pc / L.nx) % L.ny), k = (int)(pc / ((long long)L.nx * L.ny));
    const float x = L.ox + (float)i * L.sx, y = L.oy + (float)j * L.sy, z = L.oz + (float)k * L.sz;
    const int t0 = min(nt, (int)blockIdx.y * per), t1 = min(nt, t0 + per);
    float best = INFINITY;
    double angles = 0.0;
    for (int base = t0; base < t1; base += kMeshChunk) {            // (block-uniform)
        const int cnt = min(kMeshChunk, t1 - base);
        __syncthreads();
        if ((int)threadIdx.x < cnt) mesh_tri_setup(verts, tris + 3 * (size_t)(base + threadIdx.x), st[threadIdx.x]);
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const MeshTri& T = st[t];
            const float d2 = mesh_tri_d2(T, x, y, z);
            if (d2 < best) best = d2;
            angles += (double)mesh_tri_angle(T, x, y, z);
        }
    }
    if (valid) {
        d2part[(size_t)blockIdx.y * (size_t)L.total + (size_t)p] = best;
        wpart[(size_t)blockIdx.y * (size_t)L.total + (size_t)p] = angles;
    }
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_merge(const float* __restrict__ d2part, const double* __restrict__ wpart, int splits,
                                                           long long total, float* __restrict__ out) {
    const long long p = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
    if (p >= total) return;
    float best = d2part[p];
    double angles = wpart[p];
    for (int s = 1; s < splits; ++s) {
        const float d2 = d2part[(size_t)s * (size_t)total + (size_t)p];
        if (d2 < best) best = d2;
        angles += wpart[(size_t)s * (size_t)total + (size_t)p];
    }
    out[p] = mesh_signed(best, angles);
}

// ---- moments of a lattice body --------------------------------------------
// Sum over the lattice points of w {1, x, y, z, xx, yy, zz, xy, xz, yz}: x, y, z the fp32 local coordinates widened to fp64,
// w = clamp(0.5f - phi / D, 0, 1) with D the fp32 cell diagonal (a NaN phi weighs 0), the products in fp64 from the left.
//   k_volume_moments         a FIXED grid (min(kMomGrid, sweeps for the point count)) of sweeps of kMomSweep points: a thread takes four
//                            consecutive points per float4 load, kMomUnroll loads in flight; ten fp64 sums per thread, an xor butterfly per
//                            wave, the waves of a block in order, one partial row per block.
//   k_volume_moments_finish  one block: thread (chunk, term) sums a contiguous range of rows in ascending order, thread `term` the chunks
//                            in order, times the cell volume.
// No float atomic: the bits depend on the lattice only.
constexpr int kMomTerms = 10;
constexpr int kMomBlock = 256;
constexpr int kMomVec = 4;                   // consecutive points per thread and load (one float4)
constexpr int kMomUnroll = 2;                // float4 loads in flight per thread
constexpr int kMomSweep = kMomBlock * kMomUnroll * kMomVec;
constexpr int kMomGrid = 1024;               // rows of the partial slab at most (4 blocks per compute unit)
constexpr int kMomWaves = kMomBlock / 64;
constexpr int kMomFinishBlock = 1024;
constexpr int kMomChunks = kMomFinishBlock / kMomTerms;

__host__ __device__ inline float vol_diagonal(const float* spacing) {
    return sqrtf(dot3(spacing[0], spacing[1], spacing[2], spacing[0], spacing[1], spacing[2]));
}
// The ten terms of one lattice point added to t.
__host__ __device__ inline void vol_moment_terms(float phi, float diag, float lx, float ly, float lz, double (&t)[kMomTerms]) {
    const float wf = fminf(fmaxf(0.5f - phi / diag, 0.0f), 1.0f);
    const double w = (double)wf, x = (double)lx, y = (double)ly, z = (double)lz;
    const double wx = w * x, wy = w * y, wz = w * z;
    t[0] += w; t[1] += wx; t[2] += wy; t[3] += wz;
    t[4] += wx * x; t[5] += wy * y; t[6] += wz * z;
    t[7] += wx * y; t[8] += wx * z; t[9] += wy * z;
}

__global__ __launch_bounds__(kMomBlock) void k_volume_moments(VolRec v, float diag, unsigned total, double* __restrict__ part) {
    __shared__ double sacc[kMomWaves][kMomTerms];
    double t[kMomTerms];
#pragma unroll
    for (int c = 0; c < kMomTerms; ++c) t[c] = 0.0;
    const unsigned nx = (unsigned)v.dims[0], ny = (unsigned)v.dims[1];
    for (unsigned long long base = (unsigned long long)blockIdx.x * kMomSweep; base < total; base += (unsigned long long)gridDim.x * kMomSweep) {   // (block-uniform)
        float phi[kMomUnroll][kMomVec];
#pragma unroll
        for (int j = 0; j < kMomUnroll; ++j) {
            const unsigned long long p0 = base + (unsigned long long)(j * kMomBlock + (int)threadIdx.x) * kMomVec;
            if (p0 + kMomVec <= total) {                             // (the lattice starts on an allocation boundary: p0 is a multiple of four)
                const float4 q = *reinterpret_cast<const float4*>(v.values + p0);
                phi[j][0] = q.x; phi[j][1] = q.y; phi[j][2] = q.z; phi[j][3] = q.w;
            } else {
#pragma unroll
                for (int u = 0; u < kMomVec; ++u) phi[j][u] = p0 + u < total ? v.values[p0 + u] : INFINITY;   // (beyond the lattice: weight 0)
            }
        }
#pragma unroll
        for (int j = 0; j < kMomUnroll; ++j) {
            const unsigned long long p0 = base + (unsigned long long)(j * kMomBlock + (int)threadIdx.x) * kMomVec;
            if (p0 >= total) continue;
            const unsigned p = (unsigned)p0, row = p / nx, k0 = row / ny;
            unsigned i = p - row * nx, jj = row - k0 * ny, k = k0;     // one division pair per four points, then a carry
#pragma unroll
            for (int u = 0; u < kMomVec; ++u) {
                if (p0 + u < total)
                    vol_moment_terms(phi[j][u], diag, (float)i * v.spacing[0] - v.half[0], (float)jj * v.spacing[1] - v.half[1],
                                     (float)k * v.spacing[2] - v.half[2], t);
                if (++i == nx) { i = 0; if (++jj == ny) { jj = 0; ++k; } }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kMomTerms; ++c)
        for (int o = 32; o >= 1; o >>= 1) t[c] += __shfl_xor(t[c], o, 64);   // (open-coded: wave_sum per term reorders the independent chains; profiles/r20_header_refactor_ab.json)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int c = 0; c < kMomTerms; ++c) sacc[wave][c] = t[c];
    __syncthreads();
    if (threadIdx.x < kMomTerms) {
        double r = sacc[0][threadIdx.x];
        for (int w = 1; w < kMomWaves; ++w) r += sacc[w][threadIdx.x];
        part[(size_t)blockIdx.x * kMomTerms + threadIdx.x] = r;
    }
}

__global__ __launch_bounds__(kMomFinishBlock) void k_volume_moments_finish(const double* __restrict__ part, int rows, double cell, double* __restrict__ out) {
    __shared__ double sums[kMomChunks * kMomTerms];
    const int chunks = max(1, min(kMomChunks, rows));
    const int t = threadIdx.x, c = t % kMomTerms, ch = t / kMomTerms;
    if (ch < chunks) {
        const int per = (rows + chunks - 1) / chunks;
        const int r1 = min(rows, (ch + 1) * per);
        double s = 0.0;
        for (int r = ch * per; r < r1; ++r) s += part[(size_t)r * kMomTerms + c];
        sums[ch * kMomTerms + c] = s;
    }
    __syncthreads();
    if (t < kMomTerms) {
        double s = sums[t];
        for (int k = 1; k < chunks; ++k) s += sums[k * kMomTerms + t];
        out[t] = s * cell;
    }
}

}  // namespace sph
