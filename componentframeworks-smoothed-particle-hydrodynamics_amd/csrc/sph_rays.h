// sph_rays.h -- ray casts against the particles: the first sphere of radius r a ray enters (no reference counterpart; DESIGN.md
// section 3n).
//
// Every participating record is a solid sphere of radius r, 0 < r <= cellSize / 2, around its position.  A record takes part when
// ray_in_grid holds (k_bin's cell formula WITHOUT its clamp lies inside the grid on every axis: records outside the grid's box sit in
// clamped boundary cells far from where they are, and no walk along a ray could find them).  A candidate j is accepted by ray_hit with
// its entry parameter t, tmin <= t <= tmax, and has the key (ordered(t) << 32) | id_j, ordered() the sign-flip map from float bits to
// unsigned order.  The result of a ray is its smallest key: one answer whatever the order in which the candidates are met.
//
//   ray_setup / ray_hit / ray_in_grid / ray_key / ray_write    __host__ __device__: sph_rays_host (brute force over all records, no
//                             grid) runs the same functions.  The arithmetic is the contract's: every operation rounded on its own
//                             except the explicit fmaf()s, 1/a by IEEE division, sqrtf correctly rounded (hipcc's defaults on
//                             the device, the host compiler's on the host).
//   ray_walk                  __host__ __device__ too: the grid walk of one ray, given the grid through callables; sph_rays_walk_host
//                             runs it on the host over a grid built there, so the walk itself is tested without a device.
//   k_rays_bin, k_rays_order  coherence: a counting sort of the rays by the grid cell of their point of entry (the engine's scan kernels in
//                             between), so that the lanes of a wave start in the same cell: SPH_OPT_RAYS_VARIANT 1 (the default casts in the caller's order; section 6
//                             has what either costs)
//   k_rays                    one ray per lane, ray_walk over the engine's grid.  The segment [tmin, tmax] is clipped to the grid's box widened by one cell on every side
//                             (to t0 .. t1), and a 3-D DDA walks the cells with indices in [-1, dims] along it; at each step the members
//                             of the 3 x 3 x 3 block around the current cell (neighbor_rows with s = 1, which clamps the block to the
//                             cells that exist) are tested with ray_hit and the smallest key stays in registers.  No LDS, no scratch.
//   ray_span / ray_span_walk / k_ray_spans    spans, at the end of this file: what a ray crosses in all (count, first entry, last exit,
//                             summed chord share), from a walk that cannot stop early and meets every sphere exactly once
//
// Completeness.  A sphere the ray enters at t has its centre within r <= cellSize / 2 of the point P(t) of the ray.  If P(t) lies in
// cell c, the centre lies in [c - 1/2, c + 3/2) cells on every axis, inside the block of c, and it is still inside the block of any cell
// whose extent is within half a cell of P(t): that half cell is the slack for the rounding of the walk's own numbers.  Spheres stick out
// of the box by at most half a cell, so every hit point lies inside the widened box.  The walk steps through face-connected cells; where
// the ray passes a cell corner or runs along a face, whichever order it takes, the block covers the cell it skips.
// The walk's parameters do not accumulate: with P0 = o + t0 d the point of entry and G = (P0 - gridMin) / cellSize, the crossing of the
// integer plane b of an axis is at u = (b - G) * (cellSize / d) past t0, computed afresh from b at every step (two roundings, whatever
// the number of steps before).  Zero direction components never cross (u = +inf); the step count is bounded by gx + gy + gz + 6, the
// number of cells a monotone path through [-1, dims]^3 can cross.
//
// Termination.  All cells the walk has visited cover the ray up to the entry parameter tc = t0 + u of the current cell, so a sphere that
// has not been a candidate yet is entered after tc (less the rounding slack).  Once the best accepted t is below tc - margin no later
// candidate can have a smaller key, and the walk stops.  margin = (cellSize / 4) / max |d_axis|: a quarter of a cell along the fastest
// axis, in units of t; the rounding it has to cover (a few ulp of t0 + u and of the twin's t) is below 1e-5 of that for any ray whose
// points are representable to a small fraction of a cell.  SPH_RAYS_ANY_HIT stops at the first accepted candidate.
//
// Domain of the guarantee: the walk finds what the twin finds while the fp32 rounding of the ray's own points (of o, and of t * d along
// the part of the ray inside the widened box) stays below a quarter cell.  For origins millions of cells away the twin is still the
// definition, but its L = x_j - o is then itself coarser than a cell.
//
// Participation and SPH_RAYS_FLUID_ONLY are evaluated only for a candidate that ray_hit accepted with a key below the best so far, so
// the three divisions of ray_in_grid run for a handful of candidates per ray, not per candidate.
// The range guards (i < m, j < end <= n, cell indices clamped to [-1, dims] while still floats, so NaN and inf never reach an integer)
// stay so that no load or store can leave its array.
#pragma once
#include <math.h>
#include <string.h>

#include "sph_query.h"   // neighbor_rows, slot_ghost

namespace sph {

constexpr int kRaysFluidOnly = 1, kRaysAnyHit = 2;      // SPH_RAYS_* of sph_abi.h
constexpr unsigned long long kRayNoKey = ~0ull;         // above every key: ordered(t) <= ordered(+inf) = 0xff800000

struct RayK {
    float r2, invr;          // r * r in fp32; 1 / r, computed once on the host
    int flags;
    uint32_t idBase, n;      // n == 0: no record, no grid array is read
};

// One ray as the kernels and the twin see it: void rays are misses.
struct Ray {
    float ox, oy, oz, tmin, dx, dy, dz, tmax, inva;
};

__host__ __device__ inline uint32_t ray_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// float bits -> unsigned order (negative t below positive t), and back.
__host__ __device__ inline uint32_t ray_ordered(float f) {
    const uint32_t u = ray_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ray_unordered(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__host__ __device__ inline unsigned long long ray_key(float t, uint32_t id) { return ((unsigned long long)ray_ordered(t) << 32) | (unsigned long long)id; }

// Fills R from the two float4 of a ray; false: the ray is void (a non-finite o, d or tmin, a NaN tmax, a = dot3(d, d) zero or not
// finite, tmin > tmax).
__host__ __device__ inline bool ray_setup(const float* a8, Ray& R) {
    R.ox = a8[0]; R.oy = a8[1]; R.oz = a8[2]; R.tmin = a8[3];
    R.dx = a8[4]; R.dy = a8[5]; R.dz = a8[6]; R.tmax = a8[7];
    R.inva = 0.0f;
    if (!(float_finite(R.ox) && float_finite(R.oy) && float_finite(R.oz) && float_finite(R.dx) && float_finite(R.dy) && float_finite(R.dz) && float_finite(R.tmin))) return false;
    if (R.tmax != R.tmax) return false;
    const float a = dot3(R.dx, R.dy, R.dz, R.dx, R.dy, R.dz);
    if (!(a > 0.0f) || !float_finite(a)) return false;
    if (R.tmin > R.tmax) return false;
    R.inva = 1.0f / a;
    return true;
}

// Does the ray enter the sphere of squared radius r2 around (x, y, z) inside its window?  t: the entry parameter.  The projected form
// (the foot of the centre on the ray, then the half chord) does not cancel for far origins as b^2 - ac does.  Only entries count: a
// sphere that contains the ray's start has t < tmin and is not hit.  A NaN anywhere fails the compares.
__host__ __device__ inline bool ray_hit(const Ray& R, float r2, float x, float y, float z, float& t) {
    const float Lx = x - R.ox, Ly = y - R.oy, Lz = z - R.oz;
    const float tca = dot3(Lx, Ly, Lz, R.dx, R.dy, R.dz) * R.inva;
    const float qx = fmaf(-tca, R.dx, Lx), qy = fmaf(-tca, R.dy, Ly), qz = fmaf(-tca, R.dz, Lz);
    const float d2 = dot3(qx, qy, qz, qx, qy, qz);
    const float s = r2 - d2;
    if (s < 0.0f) return false;
    const float thc = sqrtf(s * R.inva);
    t = tca - thc;
    return R.tmin <= t && t <= R.tmax;
}

// k_bin's cell formula without its clamp, inside the grid on every axis.
__host__ __device__ inline bool ray_axis_in(float p, float gmin, float cellSize, int dim) {
    const float f = floorf((p - gmin) / cellSize);
    return f >= 0.0f && f < (float)dim;
}
__host__ __device__ inline bool ray_in_grid(const SimK& k, float x, float y, float z) {
    return ray_axis_in(x, k.gminx, k.cellSize, k.gx) && ray_axis_in(y, k.gminy, k.cellSize, k.gy) && ray_axis_in(z, k.gminz, k.cellSize, k.gz);
}

// The 8 words of a SphRayHit: (t, id, pos[3], normal[3]).  key == kRayNoKey: a miss; (x, y, z): the position of record id.
__host__ __device__ inline void ray_write(const Ray& R, const RayK& rk, unsigned long long key, float x, float y, float z, float* out8) {
    const float inf = ray_unordered(0xFF800000u);
    const int32_t miss = -1, zero = 0;
    for (int w = 0; w < 8; ++w) out8[w] = 0.0f;
    if (key == kRayNoKey) {
        out8[0] = inf;
        memcpy(out8 + 1, &miss, 4);
        return;
    }
    if (rk.flags & kRaysAnyHit) {
        memcpy(out8 + 1, &zero, 4);
        return;
    }
    const float t = ray_unordered((uint32_t)(key >> 32));
    const int32_t id = (int32_t)(uint32_t)(key & 0xffffffffull);
    const float px = fmaf(t, R.dx, R.ox), py = fmaf(t, R.dy, R.oy), pz = fmaf(t, R.dz, R.oz);
    out8[0] = t;
    memcpy(out8 + 1, &id, 4);
    out8[2] = px; out8[3] = py; out8[4] = pz;
    out8[5] = (px - x) * rk.invr; out8[6] = (py - y) * rk.invr; out8[7] = (pz - z) * rk.invr;
}

// Clips [t0, t1] to lo <= o + t d <= hi along one axis; false: nothing is left.
__host__ __device__ inline bool ray_clip_axis(float o, float d, float lo, float hi, float& t0, float& t1) {
    if (d == 0.0f) return o >= lo && o <= hi;
    const float ta = (lo - o) / d, tb = (hi - o) / d;
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}
// Cell coordinate of a point of the walk, clamped to [-1, dim] while still a float (NaN -> -1).
__host__ __device__ inline int ray_cell(float g, int dim) { return (int)fminf(fmaxf(floorf(g), -1.0f), (float)dim); }
// Parameter past t0 at which an axis leaves cell c: the integer plane c + 1 (d > 0) or c (d < 0); never for d == 0.
__host__ __device__ inline float ray_cross(int c, float g, float d, float cellOverD) {
    if (d == 0.0f) return INFINITY;
    return ((float)(d > 0.0f ? c + 1 : c) - g) * cellOverD;
}

// The part of [tmin, tmax] inside the grid's box widened by one cell, t0 .. t1, and the point of entry P(t0) in cell units; false:
// nothing of the ray is inside.
__host__ __device__ inline bool ray_enter(const SimK& k, const Ray& R, float& t0, float& t1, float& gX, float& gY, float& gZ) {
    const float cs = k.cellSize;
    t0 = R.tmin; t1 = R.tmax;
    if (!(ray_clip_axis(R.ox, R.dx, k.gminx - cs, fmaf((float)(k.gx + 1), cs, k.gminx), t0, t1) &&
          ray_clip_axis(R.oy, R.dy, k.gminy - cs, fmaf((float)(k.gy + 1), cs, k.gminy), t0, t1) &&
          ray_clip_axis(R.oz, R.dz, k.gminz - cs, fmaf((float)(k.gz + 1), cs, k.gminz), t0, t1) && t0 <= t1 && float_finite(t0))) return false;
    gX = (fmaf(t0, R.dx, R.ox) - k.gminx) / cs; gY = (fmaf(t0, R.dy, R.oy) - k.gminy) / cs; gZ = (fmaf(t0, R.dz, R.oz) - k.gminz) / cs;
    return true;
}

// The walk of one ray that ray_setup passed: the smallest key (kRayNoKey: a miss) and the sorted slot that holds it.  The grid comes
// in through three callables, so that sph_rays_walk_host runs this very function over a grid built on the host:
//   rows(cx, cy, cz, f)   f(first slot, end slot) per row of the 3 x 3 x 3 block around the cell, clamped to the cells that exist
//   pos(j)                float4 whose x, y, z are the position of sorted slot j
//   id(j), ghost(j)       particle id of the slot; is it a ghost (read under SPH_RAYS_FLUID_ONLY only)
template <class Rows, class Pos, class Id, class Ghost>
__host__ __device__ inline unsigned long long ray_walk(const SimK& k, const RayK& rk, const Ray& R, Rows&& rows, Pos&& pos, Id&& id, Ghost&& ghost,
                                                       uint32_t& bestSlot) {
    const bool fluidOnly = (rk.flags & kRaysFluidOnly) != 0, anyHit = (rk.flags & kRaysAnyHit) != 0;
    unsigned long long best = kRayNoKey;
    bestSlot = 0u;
    if (!rk.n) return best;
    const float cs = k.cellSize;
    float t0, t1, gX, gY, gZ;
    if (!ray_enter(k, R, t0, t1, gX, gY, gZ)) return best;
    int cx = ray_cell(gX, k.gx), cy = ray_cell(gY, k.gy), cz = ray_cell(gZ, k.gz);
    const float cdx = cs / R.dx, cdy = cs / R.dy, cdz = cs / R.dz;                          // (+-inf for a zero component: never used)
    const int sx = R.dx > 0.0f ? 1 : -1, sy = R.dy > 0.0f ? 1 : -1, sz = R.dz > 0.0f ? 1 : -1;
    const float margin = (0.25f * cs) / fmaxf(fmaxf(fabsf(R.dx), fabsf(R.dy)), fabsf(R.dz));
    const float uEnd = t1 - t0;
    float u = 0.0f;                                                                         // entry of the current cell, past t0
    const int maxSteps = k.gx + k.gy + k.gz + 6;
    for (int step = 0; step <= maxSteps; ++step) {
        if (best != kRayNoKey && (anyHit || ray_unordered((uint32_t)(best >> 32)) < (t0 + u) - margin)) break;
        rows(cx, cy, cz, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                if (anyHit && best != kRayNoKey) break;
                const float4 J = pos(j);
                float t;
                if (!ray_hit(R, rk.r2, J.x, J.y, J.z, t)) continue;
                if (ray_ordered(t) > (uint32_t)(best >> 32)) continue;
                const unsigned long long key = ray_key(t, id(j));
                if (key >= best) continue;
                if (fluidOnly && ghost(j)) continue;
                if (!ray_in_grid(k, J.x, J.y, J.z)) continue;
                best = key;
                bestSlot = j;
            }
        });
        const float ux = ray_cross(cx, gX, R.dx, cdx), uy = ray_cross(cy, gY, R.dy, cdy), uz = ray_cross(cz, gZ, R.dz, cdz);
        const float un = fminf(fminf(ux, uy), uz);
        if (!(un <= uEnd)) break;                                                           // the segment ends inside this cell (or never leaves it)
        if (ux <= uy && ux <= uz) { cx += sx; if (cx < -1 || cx > k.gx) break; }
        else if (uy <= uz) { cy += sy; if (cy < -1 || cy > k.gy) break; }
        else { cz += sz; if (cz < -1 || cz > k.gz) break; }
        u = fmaxf(u, un);
    }
    return best;
}

// (hits, void rays) of the wave into stats[0], stats[1]: every lane of the wave must arrive.
__device__ __forceinline__ void rays_reduce(bool hit, bool isVoid, unsigned long long* __restrict__ stats) {
    const unsigned long long nh = (unsigned long long)__popcll(__ballot(hit)), nv = (unsigned long long)__popcll(__ballot(isVoid));
    if ((threadIdx.x & 63) == 0) {
        if (nh) atomicAdd(stats + 0, nh);
        if (nv) atomicAdd(stats + 1, nv);
    }
}

// Ray i -> bin[i] = (the grid cell of its point of entry, clamped into the grid; numCells for a ray that is void or passes the widened
// box by, which has no walk), its arrival number among the rays of that cell); count[0 .. numCells] must be zero and comes back
// as the histogram.  The arrival numbers of a cell depend on the run; the hits do not: they are written by ray index.
__global__ __launch_bounds__(kBlock) void k_rays_bin(SimK k, const float4* __restrict__ rays, size_t m, uint2* __restrict__ bin, uint32_t* __restrict__ count) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 A = rays[2 * i], B = rays[2 * i + 1];
    const float a8[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    Ray R;
    uint32_t key = (uint32_t)k.numCells;
    float t0, t1, gX, gY, gZ;
    if (ray_setup(a8, R) && ray_enter(k, R, t0, t1, gX, gY, gZ)) {
        const int cx = min(max(ray_cell(gX, k.gx), 0), k.gx - 1), cy = min(max(ray_cell(gY, k.gy), 0), k.gy - 1), cz = min(max(ray_cell(gZ, k.gz), 0), k.gz - 1);
        key = (uint32_t)((cz * k.gy + cy) * k.gx + cx);
    }
    bin[i] = make_uint2(key, atomicAdd(count + key, 1u));
}
// order[start[cell] + arrival number] = i: the rays in the order of their cell of entry.  (start[] ends at m; the guard stays.)
__global__ __launch_bounds__(kBlock) void k_rays_order(const uint2* __restrict__ bin, const uint32_t* __restrict__ start, size_t m, uint32_t* __restrict__ order) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint2 b = bin[i];
    const size_t at = (size_t)start[b.x] + b.y;
    if (at < m) order[at] = (uint32_t)i;
}

// order: the ray of every lane (k_rays_order), or null for the caller's order.
__global__ __launch_bounds__(kBlock) void k_rays(SimK k, RayK rk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                 const float4* __restrict__ own, const float4* __restrict__ rays, const uint32_t* __restrict__ order, size_t m,
                                                 float4* __restrict__ hits, unsigned long long* __restrict__ stats) {
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t i = (order && lane < m) ? (size_t)order[lane] : lane;
    const bool act = lane < m && i < m;
    Ray R;
    bool live = false;
    if (act) {
        const float4 A = rays[2 * i], B = rays[2 * i + 1];
        const float a8[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        live = ray_setup(a8, R);
    }
    unsigned long long best = kRayNoKey;
    uint32_t bestSlot = 0u;
    if (live)
        best = ray_walk(
            k, rk, R, [&](int cx, int cy, int cz, auto&& f) { neighbor_rows(k, cellStart, 1, rk.n, cx, cy, cz, f); }, [&](uint32_t j) { return pv[2u * j]; },
            [&](uint32_t j) { const uint32_t id = fbits(own[j].w) - rk.idBase; return id < rk.n ? id : 0u; }, [&](uint32_t j) { return slot_ghost(own, j); }, bestSlot);
    if (act) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (best != kRayNoKey && !(rk.flags & kRaysAnyHit)) {
            const float4 J = pv[2u * bestSlot];
            x = J.x; y = J.y; z = J.z;
        }
        float o8[8];
        ray_write(R, rk, best, x, y, z, o8);
        hits[2 * i] = make_float4(o8[0], o8[1], o8[2], o8[3]);
        hits[2 * i + 1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
    }
    rays_reduce(act && best != kRayNoKey, act && !live, stats);
}

// ---- spans: what a ray crosses in all (DESIGN.md section 3n "Spans") ------------------------------------------------------------
// Per ray the number of spheres whose chord inside [tmin, tmax] has positive length, the smallest tin and the largest tout with the ids
// that hold them, and the summed chord length in units of 2^-24 of a diameter.  Every field is a min, a max or an integer sum of
// per-sphere values (ray_span) that do not depend on how the sphere was found: sph_rays_span_host (brute force, no grid) is the
// definition and a walk gives its bytes as long as it hands every participating sphere to ray_span exactly once.
//
// Completeness is the cast's: the part of a chord inside the window has positive length and lies in the widened box (centres are
// inside the grid, r is at most half a cell), hence in [t0, t1]; each of its points is within r of the centre, so the centre is in the
// block of the cell that holds the point.  The walk has no termination test: it ends with the segment or outside [-1, dims].
// Once only.  The DDA's path is monotone per axis, and cell X lies in block(c) iff |X - c| <= 1 on every axis: a box of cells, which a
// monotone path meets in ONE contiguous run.  X is therefore new exactly at the step that enters the run.
//   layer walk   the first cell tests its whole block; after a step of s = +-1 along axis a only the cells with coordinate c_a + s of
//                the new block are tested: that layer is block(c_new) \ block(c_prev), so nothing is tested twice, and the step that
//                enters X's run has X_a = c_a + s, so nothing is left out.  A third of the candidates.
//   block walk   every step tests the whole block (as k_rays), and a crossed candidate is dropped when its own cell (the floor of
//                ray_axis_in, which participation computes anyway; for a participant it is the cell the grid holds it in) lies within
//                Chebyshev distance 1 of the PREVIOUS cell of the path: "in the previous block" is "seen before" by the run argument.
//                Integers only.

struct RaySpanAcc {
    unsigned long long enter = kRayNoKey;    // smallest (ordered(tin) << 32) | id
    unsigned long long exit = 0ull;          // largest (ordered(tout) << 32) | ~id: ties go to the smaller id; below every real key
    unsigned long long length = 0ull;
    uint32_t count = 0u;
};

// Is the sphere crossed?  tca, thc as ray_hit forms them; the chord clipped to the window; q its share of the diameter in 2^-24.
__host__ __device__ inline bool ray_span(const Ray& R, float r2, float x, float y, float z, float& tin, float& tout, uint32_t& q) {
    const float Lx = x - R.ox, Ly = y - R.oy, Lz = z - R.oz;
    const float tca = dot3(Lx, Ly, Lz, R.dx, R.dy, R.dz) * R.inva;
    const float qx = fmaf(-tca, R.dx, Lx), qy = fmaf(-tca, R.dy, Ly), qz = fmaf(-tca, R.dz, Lz);
    const float d2 = dot3(qx, qy, qz, qx, qy, qz);
    const float s = r2 - d2;
    if (!(s >= 0.0f)) return false;
    const float thc = sqrtf(s * R.inva);
    tin = fmaxf(tca - thc, R.tmin);
    tout = fminf(tca + thc, R.tmax);
    if (!(tin < tout)) return false;
    const float f = fminf((tout - tin) / (2.0f * thc), 1.0f);
    q = (uint32_t)fmaf(f, 16777216.0f, 0.5f);
    return true;
}
__host__ __device__ inline void ray_span_add(RaySpanAcc& a, float tin, float tout, uint32_t q, uint32_t id) {
    const unsigned long long ke = ray_key(tin, id), kx = ((unsigned long long)ray_ordered(tout) << 32) | (unsigned long long)(~id);
    a.enter = ke < a.enter ? ke : a.enter;
    a.exit = kx > a.exit ? kx : a.exit;
    a.length += q;
    a.count += 1u;
}
// ray_in_grid with the integer cell its floors give; the cell is meaningful where the result is true.
__host__ __device__ inline bool ray_cell_in(const SimK& k, float x, float y, float z, int& X, int& Y, int& Z) {
    const float fx = floorf((x - k.gminx) / k.cellSize), fy = floorf((y - k.gminy) / k.cellSize), fz = floorf((z - k.gminz) / k.cellSize);
    if (!(fx >= 0.0f && fx < (float)k.gx && fy >= 0.0f && fy < (float)k.gy && fz >= 0.0f && fz < (float)k.gz)) return false;
    X = (int)fx; Y = (int)fy; Z = (int)fz;
    return true;
}

// The 8 words of a SphRaySpan: (tEnter, tExit, idEnter, idExit, count, flags, length lo, length hi).
__host__ __device__ inline void ray_span_write(const RaySpanAcc& a, bool isVoid, uint32_t* out8) {
    out8[0] = 0x7F800000u; out8[1] = 0xFF800000u; out8[2] = 0xFFFFFFFFu; out8[3] = 0xFFFFFFFFu;
    out8[4] = a.count; out8[5] = isVoid ? 1u : 0u;
    out8[6] = (uint32_t)(a.length & 0xffffffffull); out8[7] = (uint32_t)(a.length >> 32);
    if (!a.count) return;
    out8[0] = ray_bits(ray_unordered((uint32_t)(a.enter >> 32)));
    out8[1] = ray_bits(ray_unordered((uint32_t)(a.exit >> 32)));
    out8[2] = (uint32_t)(a.enter & 0xffffffffull);
    out8[3] = ~(uint32_t)(a.exit & 0xffffffffull);
}

// neighbor_rows for an arbitrary box of cells [x0, x1] x [y0, y1] x [z0, z1], clamped to the cells that exist: f(first slot, end slot)
// per row, ascending.
template <class F>
__host__ __device__ __forceinline__ void cell_box_rows(const SimK& k, const uint32_t* __restrict__ cellStart, uint32_t n, int x0, int x1, int y0, int y1, int z0, int z1,
                                                       F&& f) {
    x0 = max(x0, 0); x1 = min(x1, k.gx - 1);
    y0 = max(y0, 0); y1 = min(y1, k.gy - 1);
    z0 = max(z0, 0); z1 = min(z1, k.gz - 1);
    if (x0 > x1) return;
    for (int nz = z0; nz <= z1; ++nz)
        for (int ny = y0; ny <= y1; ++ny) {
            const int rowBase = (nz * k.gy + ny) * k.gx;
            f(cellStart[rowBase + x0], min(cellStart[rowBase + x1 + 1], n));
        }
}

// The span walk of one ray that ray_setup passed.  BLOCK: the block walk, else the layer walk.  The grid through callables as in
// ray_walk, with rows(x0, x1, y0, y1, z0, z1, f) the rows of a box of cells (cell_box_rows).
template <bool BLOCK, class Rows, class Pos, class Id, class Ghost>
__host__ __device__ inline void ray_span_walk(const SimK& k, const RayK& rk, const Ray& R, Rows&& rows, Pos&& pos, Id&& id, Ghost&& ghost, RaySpanAcc& acc) {
    const bool fluidOnly = (rk.flags & kRaysFluidOnly) != 0;
    if (!rk.n) return;
    const float cs = k.cellSize;
    float t0, t1, gX, gY, gZ;
    if (!ray_enter(k, R, t0, t1, gX, gY, gZ)) return;
    int cx = ray_cell(gX, k.gx), cy = ray_cell(gY, k.gy), cz = ray_cell(gZ, k.gz);
    const float cdx = cs / R.dx, cdy = cs / R.dy, cdz = cs / R.dz;
    const int sx = R.dx > 0.0f ? 1 : -1, sy = R.dy > 0.0f ? 1 : -1, sz = R.dz > 0.0f ? 1 : -1;
    const float uEnd = t1 - t0;
    int px = -4, py = -4, pz = -4;                                                          // the previous cell of the path: none yet (no cell of the grid is near -4)
    int x0 = cx - 1, x1 = cx + 1, y0 = cy - 1, y1 = cy + 1, z0 = cz - 1, z1 = cz + 1;       // the box of cells to test at this step
    const int maxSteps = k.gx + k.gy + k.gz + 6;
    for (int step = 0; step <= maxSteps; ++step) {
        rows(x0, x1, y0, y1, z0, z1, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                const float4 J = pos(j);
                float tin, tout;
                uint32_t q;
                if (!ray_span(R, rk.r2, J.x, J.y, J.z, tin, tout, q)) continue;
                if (fluidOnly && ghost(j)) continue;
                int X, Y, Z;
                if (!ray_cell_in(k, J.x, J.y, J.z, X, Y, Z)) continue;
                if (BLOCK && abs(X - px) <= 1 && abs(Y - py) <= 1 && abs(Z - pz) <= 1) continue;
                ray_span_add(acc, tin, tout, q, id(j));
            }
        });
        const float ux = ray_cross(cx, gX, R.dx, cdx), uy = ray_cross(cy, gY, R.dy, cdy), uz = ray_cross(cz, gZ, R.dz, cdz);
        const float un = fminf(fminf(ux, uy), uz);
        if (!(un <= uEnd)) break;                                                           // the segment ends inside this cell (or never leaves it)
        px = cx; py = cy; pz = cz;
        if (ux <= uy && ux <= uz) { cx += sx; if (cx < -1 || cx > k.gx) break; }
        else if (uy <= uz) { cy += sy; if (cy < -1 || cy > k.gy) break; }
        else { cz += sz; if (cz < -1 || cz > k.gz) break; }
        x0 = cx - 1; x1 = cx + 1; y0 = cy - 1; y1 = cy + 1; z0 = cz - 1; z1 = cz + 1;
        if (!BLOCK) {                                                                       // the new layer only
            if (cx != px) x0 = x1 = cx + sx;
            else if (cy != py) y0 = y1 = cy + sy;
            else z0 = z1 = cz + sz;
        }
    }
}

// One ray per lane, order as in k_rays.  The two keys, the length and the count stay in registers; spans[2 i], spans[2 i + 1]: the
// 32 bytes of ray i.  stats: crossed rays, void rays, the sum of the counts (added), the largest count (max), reduced per wave first.
template <bool BLOCK>
__global__ __launch_bounds__(kBlock) void k_ray_spans(SimK k, RayK rk, const float4* __restrict__ pv, const uint32_t* __restrict__ cellStart,
                                                      const float4* __restrict__ own, const float4* __restrict__ rays, const uint32_t* __restrict__ order, size_t m,
                                                      uint4* __restrict__ spans, unsigned long long* __restrict__ stats) {
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t i = (order && lane < m) ? (size_t)order[lane] : lane;
    const bool act = lane < m && i < m;
    Ray R;
    bool live = false;
    if (act) {
        const float4 A = rays[2 * i], B = rays[2 * i + 1];
        const float a8[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        live = ray_setup(a8, R);
    }
    RaySpanAcc acc;
    if (live)
        ray_span_walk<BLOCK>(
            k, rk, R, [&](int x0, int x1, int y0, int y1, int z0, int z1, auto&& f) { cell_box_rows(k, cellStart, rk.n, x0, x1, y0, y1, z0, z1, f); },
            [&](uint32_t j) { return pv[2u * j]; }, [&](uint32_t j) { const uint32_t id = fbits(own[j].w) - rk.idBase; return id < rk.n ? id : 0u; },
            [&](uint32_t j) { return slot_ghost(own, j); }, acc);
    if (act) {
        uint32_t o8[8];
        ray_span_write(acc, !live, o8);
        spans[2 * i] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
        spans[2 * i + 1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
    }
    const uint32_t cnt = act ? acc.count : 0u;
    const unsigned long long nc = (unsigned long long)__popcll(__ballot(cnt != 0u)), nv = (unsigned long long)__popcll(__ballot(act && !live));
    const unsigned long long total = wave_sum((unsigned long long)cnt), mx = (unsigned long long)wave_max(cnt);
    if ((threadIdx.x & 63) == 0) {
        if (nc) atomicAdd(stats + 0, nc);
        if (nv) atomicAdd(stats + 1, nv);
        if (total) { atomicAdd(stats + 2, total); atomicMax(stats + 3, mx); }
    }
}

}  // namespace sph
