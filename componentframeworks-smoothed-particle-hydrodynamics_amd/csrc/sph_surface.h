// sph_surface.h -- iso-surface of a scalar lattice as a closed triangle mesh (no reference counterpart).
//
// Marching tetrahedra on the Kuhn (Freudenthal) split of the lattice: the cube whose lowest corner is point p is cut into six
// tets, one per axis order (a, b, c) in the order xyz, xzy, yxz, yzx, zxy, zyx, with corners m0 = 0, m1 = 1<<a,
// m2 = (1<<a)|(1<<b), m3 = 7.  Tet edge (mk, ml), k < l, is the lattice edge from p + offset(mk) in direction d = ml ^ mk (1..7).
// A point is inside iff f >= iso (NaN never is).  Every crossed lattice edge gets ONE vertex, shared by every tet that uses it.
//
//   k_surf_count       per point: 7-bit mask of its crossed edges (endpoint inside the lattice), its own inside bit and its
//                      cube's triangle count, packed in 16 bits; per tile of kSurfTile points: both sums
//   k_surf_scan_tiles  one block: 64-bit exclusive offsets of the tiles (vertices, triangles) and the two totals
//   k_surf_vertices    per tile, a block scan of the vertex counts: vOff[p], then position and normal of each crossed edge
//   k_surf_triangles   per tile, a block scan of the triangle counts: each cube's triangles from the constant table
//
// Output order is part of the contract (vertices by point index, then d; triangles by cube, tet, table order), so no
// global atomic places anything: every offset comes from the deterministic scans.  The table is generated at compile time
// from the rules (make_surf_table), not typed in.
#pragma once
#include "sph_sample.h"

namespace sph {

// ---- the table: 6 tets x 16 inside patterns (bit k = corner mk inside), at most 2 triangles of 3 edges each -----------------
// An edge is stored as (start corner << 3) | d.
struct SurfTable {
    uint8_t ntri[6][16];
    uint8_t tri[6][16][2][3];
};

constexpr int kSurfTetAxes[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr int surf_chain(int tet, int k) {
    return k == 0 ? 0 : k == 1 ? (1 << kSurfTetAxes[tet][0]) : k == 2 ? ((1 << kSurfTetAxes[tet][0]) | (1 << kSurfTetAxes[tet][1])) : 7;
}

// tet edge {k, l} as a lattice edge: start corner m_min, direction m_max ^ m_min
constexpr uint8_t surf_edge(int tet, int k, int l) {
    const int lo = k < l ? k : l, hi = k < l ? l : k;
    const int a = surf_chain(tet, lo), b = surf_chain(tet, hi);
    return (uint8_t)((a << 3) | (a ^ b));
}

// Twice the t = 1/2 point of an edge, in cube-corner units (integers: the winding test is exact).
constexpr int surf_mid2(uint8_t e, int axis) {
    const int c = e >> 3, d = e & 7;
    return 2 * ((c >> axis) & 1) + ((d >> axis) & 1);
}

// Appends triangle (e0, e1, e2) to slot n, flipped (second and third swapped) unless its normal (b - a) x (c - a) points along
// (mean of the outside corners - mean of the inside corners), here scaled to nIn * sum(out) - nOut * sum(in).
constexpr void surf_put(SurfTable& t, int tet, int cs, int n, uint8_t e0, uint8_t e1, uint8_t e2, const int (&dir)[3]) {
    int u[3] = {}, v[3] = {};
    for (int a = 0; a < 3; ++a) { u[a] = surf_mid2(e1, a) - surf_mid2(e0, a); v[a] = surf_mid2(e2, a) - surf_mid2(e0, a); }
    const int nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
    const bool keep = nx * dir[0] + ny * dir[1] + nz * dir[2] > 0;
    t.tri[tet][cs][n][0] = e0;
    t.tri[tet][cs][n][1] = keep ? e1 : e2;
    t.tri[tet][cs][n][2] = keep ? e2 : e1;
}

constexpr SurfTable make_surf_table() {
    SurfTable t{};
    for (int tet = 0; tet < 6; ++tet) {
        for (int cs = 0; cs < 16; ++cs) {
            int in[4] = {}, out[4] = {}, nIn = 0, nOut = 0;
            for (int k = 0; k < 4; ++k) {
                if ((cs >> k) & 1) in[nIn++] = k;
                else out[nOut++] = k;
            }
            int dir[3] = {};
            for (int a = 0; a < 3; ++a) {
                int sIn = 0, sOut = 0;
                for (int q = 0; q < nIn; ++q) sIn += (surf_chain(tet, in[q]) >> a) & 1;
                for (int q = 0; q < nOut; ++q) sOut += (surf_chain(tet, out[q]) >> a) & 1;
                dir[a] = nIn * sOut - nOut * sIn;
            }
            if (nIn == 1 || nOut == 1) {                         // the lone corner s and the other three r0 < r1 < r2 in chain order
                const int s = nIn == 1 ? in[0] : out[0];
                const int* r = nIn == 1 ? out : in;
                surf_put(t, tet, cs, 0, surf_edge(tet, s, r[0]), surf_edge(tet, s, r[1]), surf_edge(tet, s, r[2]), dir);
                t.ntri[tet][cs] = 1;
            } else if (nIn == 2) {                               // quad (i0,o0), (i0,o1), (i1,o1), (i1,o0), split along q0 - q2
                const uint8_t q0 = surf_edge(tet, in[0], out[0]), q1 = surf_edge(tet, in[0], out[1]);
                const uint8_t q2 = surf_edge(tet, in[1], out[1]), q3 = surf_edge(tet, in[1], out[0]);
                surf_put(t, tet, cs, 0, q0, q1, q2, dir);
                surf_put(t, tet, cs, 1, q0, q2, q3, dir);
                t.ntri[tet][cs] = 2;
            }
        }
    }
    return t;
}

__constant__ SurfTable c_surfTable = make_surf_table();

// ---- kernels ---------------------------------------------------------------------------------------------------------------
constexpr int kSurfItems = 16;                        // points per thread and tile row
constexpr int kSurfTile = kBlock * kSurfItems;        // 4096 points per tile (one block); point p = tile * kSurfTile + it * kBlock + tid

struct SurfK {
    float ox, oy, oz, sx, sy, sz;
    int dx, dy, dz;
    long long npts;
    float iso;
    int nTiles;
};

struct SurfVertex { float px, py, pz, nx, ny, nz; };   // SphSurfaceVertex

__device__ __forceinline__ long long surf_corner(const SurfK& s, int c) {
    return (long long)(c & 1) + (long long)((c >> 1) & 1) * s.dx + (long long)((c >> 2) & 1) * ((long long)s.dx * s.dy);
}

// Code of point p: bits 0..6 crossed edges d = 1..7 (bit d - 1), bit 7 inside(p), bits 8..11 the triangles of p's cube.
__device__ __forceinline__ uint32_t surf_code(const SurfK& s, const float* __restrict__ f, long long p) {
    const int i = (int)(p % s.dx), j = (int)((p / s.dx) % s.dy), l = (int)(p / ((long long)s.dx * s.dy));
    const bool hx = i + 1 < s.dx, hy = j + 1 < s.dy, hz = l + 1 < s.dz;
    uint32_t inBits = 0u, have = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (((c & 1) && !hx) || ((c & 2) && !hy) || ((c & 4) && !hz)) continue;
        have |= 1u << c;
        inBits |= (f[p + surf_corner(s, c)] >= s.iso ? 1u : 0u) << c;
    }
    const uint32_t in0 = inBits & 1u;
    uint32_t mask = 0u;
#pragma unroll
    for (int d = 1; d < 8; ++d)
        if (((have >> d) & 1u) && ((inBits >> d) & 1u) != in0) mask |= 1u << (d - 1);
    uint32_t ntri = 0u;
    if (have == 0xFFu) {
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) {
            const int m1 = 1 << kSurfTetAxes[tet][0], m2 = m1 | (1 << kSurfTetAxes[tet][1]);
            const uint32_t cs = in0 | (((inBits >> m1) & 1u) << 1) | (((inBits >> m2) & 1u) << 2) | (((inBits >> 7) & 1u) << 3);
            ntri += c_surfTable.ntri[tet][cs];
        }
    }
    return mask | (in0 << 7) | (ntri << 8);
}

__global__ __launch_bounds__(kBlock) void k_surf_count(SurfK s, const float* __restrict__ f, uint16_t* __restrict__ codes, uint2* __restrict__ tileSums) {
    __shared__ uint32_t sm[4];
    const long long base = (long long)blockIdx.x * kSurfTile + threadIdx.x;
    uint32_t nv = 0u, nt = 0u;
    for (int it = 0; it < kSurfItems; ++it) {
        const long long p = base + (long long)it * kBlock;
        if (p >= s.npts) break;
        const uint32_t code = surf_code(s, f, p);
        codes[p] = (uint16_t)code;
        nv += __popc(code & 0x7Fu);
        nt += code >> 8;
    }
    uint32_t totV, totT;
    (void)block_excl_scan(nv, sm, totV);
    (void)block_excl_scan(nt, sm, totT);
    if (threadIdx.x == 0) tileSums[blockIdx.x] = make_uint2(totV, totT);
}

// One block.  Thread t sums a contiguous run of tiles, the 256 run sums are scanned in 64 bits, then each thread writes its run's
// exclusive offsets: tileOff[2 t] vertices, tileOff[2 t + 1] triangles; tileOff[2 nTiles], [2 nTiles + 1] the totals.
__global__ __launch_bounds__(kBlock) void k_surf_scan_tiles(const uint2* __restrict__ tileSums, unsigned long long* __restrict__ tileOff, int nTiles) {
    __shared__ unsigned long long sm[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (nTiles + kBlock - 1) / kBlock;
    const int t0 = min(tid * per, nTiles), t1 = min(t0 + per, nTiles);
    unsigned long long sv = 0ull, st = 0ull;
    for (int t = t0; t < t1; ++t) { const uint2 q = tileSums[t]; sv += q.x; st += q.y; }
    const unsigned long long iv = wave_incl_scan64(sv), it = wave_incl_scan64(st);
    if (lane == 63) { sm[0][w] = iv; sm[1][w] = it; }
    __syncthreads();
    unsigned long long bv = iv - sv, bt = it - st;
    for (int q = 0; q < w; ++q) { bv += sm[0][q]; bt += sm[1][q]; }
    for (int t = t0; t < t1; ++t) {
        const uint2 q = tileSums[t];
        tileOff[2 * (size_t)t] = bv;
        tileOff[2 * (size_t)t + 1] = bt;
        bv += q.x; bt += q.y;
    }
    if (tid == 0) {
        unsigned long long tv = 0ull, tt = 0ull;
        for (int q = 0; q < 4; ++q) { tv += sm[0][q]; tt += sm[1][q]; }
        tileOff[2 * (size_t)nTiles] = tv;
        tileOff[2 * (size_t)nTiles + 1] = tt;
    }
}

// g_axis at a lattice point: central inside the lattice, one-sided on its first and last point; x[+-] are lattice coordinates.
__device__ __forceinline__ float surf_grad(const float* __restrict__ f, long long p, int i, int n, long long stride, float o, float sp) {
    const int lo = i > 0 ? i - 1 : i, hi = i + 1 < n ? i + 1 : i;
    const float fp = f[p + (long long)(hi - i) * stride], fm = f[p - (long long)(i - lo) * stride];
    return (fp - fm) / (lattice_coord(o, hi, sp) - lattice_coord(o, lo, sp));
}

__global__ __launch_bounds__(kBlock) void k_surf_vertices(SurfK s, const float* __restrict__ f, const uint16_t* __restrict__ codes,
                                                          const unsigned long long* __restrict__ tileOff, uint32_t* __restrict__ vOff,
                                                          SurfVertex* __restrict__ out) {
    __shared__ uint32_t sm[4];
    const long long base = (long long)blockIdx.x * kSurfTile + threadIdx.x;
    const long long sxy = (long long)s.dx * s.dy;
    uint32_t carry = (uint32_t)tileOff[2 * (size_t)blockIdx.x];
    for (int it = 0; it < kSurfItems; ++it) {
        const long long p = base + (long long)it * kBlock;
        const bool live = p < s.npts;
        const uint32_t mask = live ? (uint32_t)codes[p] & 0x7Fu : 0u;
        uint32_t total;
        uint32_t off = carry + block_excl_scan((uint32_t)__popc(mask), sm, total);
        carry += total;
        if (!live) continue;
        vOff[p] = off;
        if (!mask) continue;
        const int i = (int)(p % s.dx), j = (int)((p / s.dx) % s.dy), l = (int)(p / sxy);
        const float fa = f[p];
        const float ax = lattice_coord(s.ox, i, s.sx), ay = lattice_coord(s.oy, j, s.sy), az = lattice_coord(s.oz, l, s.sz);
        const float gax = surf_grad(f, p, i, s.dx, 1, s.ox, s.sx), gay = surf_grad(f, p, j, s.dy, s.dx, s.oy, s.sy),
                    gaz = surf_grad(f, p, l, s.dz, sxy, s.oz, s.sz);
        for (int d = 1; d < 8; ++d) {
            if (!((mask >> (d - 1)) & 1u)) continue;
            const int ib = i + (d & 1), jb = j + ((d >> 1) & 1), lb = l + ((d >> 2) & 1);
            const long long q = p + surf_corner(s, d);
            const float fb = f[q];
            const float t = (s.iso - fa) / (fb - fa);
            const float bx = lattice_coord(s.ox, ib, s.sx), by = lattice_coord(s.oy, jb, s.sy), bz = lattice_coord(s.oz, lb, s.sz);
            const float gbx = surf_grad(f, q, ib, s.dx, 1, s.ox, s.sx), gby = surf_grad(f, q, jb, s.dy, s.dx, s.oy, s.sy),
                        gbz = surf_grad(f, q, lb, s.dz, sxy, s.oz, s.sz);
            SurfVertex v;
            v.px = ax + t * (bx - ax); v.py = ay + t * (by - ay); v.pz = az + t * (bz - az);
            float nx = -(gax + t * (gbx - gax)), ny = -(gay + t * (gby - gay)), nz = -(gaz + t * (gbz - gaz));
            const float ss = (nx * nx + ny * ny) + nz * nz;
            if (ss == 0.0f) { nx = ny = nz = 0.0f; }
            else { const float r = sqrtf(ss); nx = nx / r; ny = ny / r; nz = nz / r; }
            v.nx = nx; v.ny = ny; v.nz = nz;
            float2* o = reinterpret_cast<float2*>(out + off);
            o[0] = make_float2(v.px, v.py); o[1] = make_float2(v.pz, v.nx); o[2] = make_float2(v.ny, v.nz);
            ++off;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_surf_triangles(SurfK s, const uint16_t* __restrict__ codes, const uint32_t* __restrict__ vOff,
                                                           const unsigned long long* __restrict__ tileOff, uint32_t* __restrict__ tris) {
    __shared__ uint32_t sm[4];
    const long long base = (long long)blockIdx.x * kSurfTile + threadIdx.x;
    uint32_t carry = (uint32_t)tileOff[2 * (size_t)blockIdx.x + 1];
    for (int it = 0; it < kSurfItems; ++it) {
        const long long p = base + (long long)it * kBlock;
        const uint32_t code = p < s.npts ? (uint32_t)codes[p] : 0u;
        uint32_t total;
        const uint32_t first = carry + block_excl_scan(code >> 8, sm, total);
        carry += total;
        if (!(code >> 8)) continue;                                    // (a cube with triangles has all 8 corners in the lattice)
        uint32_t cc[8];
        cc[0] = code;
#pragma unroll
        for (int c = 1; c < 8; ++c) cc[c] = codes[p + surf_corner(s, c)];
        uint32_t inBits = 0u;
#pragma unroll
        for (int c = 0; c < 8; ++c) inBits |= ((cc[c] >> 7) & 1u) << c;
        size_t k = (size_t)first * 3u;
        for (int tet = 0; tet < 6; ++tet) {
            const int m1 = 1 << kSurfTetAxes[tet][0], m2 = m1 | (1 << kSurfTetAxes[tet][1]);
            const uint32_t cs = (inBits & 1u) | (((inBits >> m1) & 1u) << 1) | (((inBits >> m2) & 1u) << 2) | (((inBits >> 7) & 1u) << 3);
            const int n = c_surfTable.ntri[tet][cs];
            for (int q = 0; q < n; ++q) {
                for (int v = 0; v < 3; ++v) {
                    const int e = c_surfTable.tri[tet][cs][q][v], c = e >> 3, d = e & 7;
                    tris[k++] = vOff[p + surf_corner(s, c)] + (uint32_t)__popc(cc[c] & ((1u << (d - 1)) - 1u));
                }
            }
        }
    }
}

}  // namespace sph
