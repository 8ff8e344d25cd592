// aniso_surface.cpp -- anisotropic kernels through the C++ twin only: the default scene gets a wave impulse, then once per frame the
// ellipsoid of every particle (Anisotropy, DownloadAniso) and the water surface twice, from the isotropic fraction (ExtractSurface) and
// from the anisotropic one (ExtractAnisoSurface), on the lattice of spacing h/2 over the grid box widened by 2h.  Prints the sparse and
// clamped counts, the mean |axis2| / |axis0| and the vertex and triangle counts of both surfaces, and checks the result: the axes of a
// valid row are mutually orthogonal, their lengths descend, |axis0| <= support * maxStretch, |axis0| / |axis2| <= maxRatio, a row
// without SPH_ANISO_VALID is all zero, the counts are those of AnisoInfo, and every undirected edge of the anisotropic mesh lies in
// exactly two triangles.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/aniso_surface.cpp -L <pkg dir> -lsph_hip -o aniso_surface
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static double Dot(const float* a, const float* b) { return double(a[0]) * b[0] + double(a[1]) * b[1] + double(a[2]) * b[2]; }

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 3;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    const float h = fluid.param_h, s = 0.5f * h;
    const Vec3 origin(fluid.gridMinV.x - 2.0f * h, fluid.gridMinV.y - 2.0f * h, fluid.gridMinV.z - 2.0f * h);
    const int gdims[3] = {fluid.gridSizeX, fluid.gridSizeY, fluid.gridSizeZ};
    int dims[3];
    for (int a = 0; a < 3; ++a) dims[a] = int(std::ceil((fluid.cellSize * float(gdims[a]) + 4.0f * h) / s)) + 1;
    const SphAnisoConfig cfg = SPHFluidGPU::AnisoConfig();
    const double support = double(h);                                  // (cfg.support 0: param_h)
    // Orthogonality: the eigenvectors are the product of 15 plane rotations in fp32.  A rotation rewrites two columns with two roundings per
    // entry (2u of the column's length, u = 2^-24), and its c, s come from two divisions, two square roots and three more operations, so
    // c^2 + s^2 misses 1 by at most about 8u: 10u per rotation, 150u after 15, and the cosine between two columns by twice that.
    const double kOrtho = 300.0 * std::ldexp(1.0, -24), kRound = 1e-5;
    std::vector<SphAniso> rows;
    std::vector<SphSurfaceVertex> verts;
    std::vector<uint32_t> tris;
    for (int frame = 0; frame < frames; ++frame) {
        for (int k = 0; k < 8; ++k) fluid.DispatchCompute(fluid.param_timeStep);
        SphAnisoInfo info;
        if (!fluid.Anisotropy(info, cfg) || !fluid.DownloadAniso(rows)) {
            std::printf("Anisotropy failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        uint64_t sparse = 0, clamped = 0, valid = 0;
        uint32_t maxCount = 0;
        float maxReach = 0.0f;
        double ratioSum = 0.0;
        static const SphAniso zero{};
        for (size_t i = 0; i < rows.size(); ++i) {
            const SphAniso& r = rows[i];
            if (!(r.flags & SPH_ANISO_VALID)) {
                if (std::memcmp(&r, &zero, sizeof(r)) != 0) { std::printf("row %zu is not valid and not all zero\n", i); return 4; }
                continue;
            }
            valid += 1;
            if (r.flags & SPH_ANISO_SPARSE) sparse += 1;
            if (r.flags & SPH_ANISO_CLAMPED) clamped += 1;
            maxCount = std::max(maxCount, r.count);
            maxReach = std::max(maxReach, r.reach);
            const double l0 = std::sqrt(Dot(r.axis0, r.axis0)), l1 = std::sqrt(Dot(r.axis1, r.axis1)), l2 = std::sqrt(Dot(r.axis2, r.axis2));
            if (!(l2 > 0.0)) { std::printf("row %zu: axis2 has no length\n", i); return 5; }
            const double c01 = std::fabs(Dot(r.axis0, r.axis1)) / (l0 * l1), c02 = std::fabs(Dot(r.axis0, r.axis2)) / (l0 * l2),
                         c12 = std::fabs(Dot(r.axis1, r.axis2)) / (l1 * l2);
            if (std::max(c01, std::max(c02, c12)) > kOrtho) { std::printf("row %zu: axes not orthogonal (%g %g %g)\n", i, c01, c02, c12); return 5; }
            if (l0 < l1 * (1.0 - kRound) || l1 < l2 * (1.0 - kRound)) { std::printf("row %zu: lengths %g %g %g do not descend\n", i, l0, l1, l2); return 6; }
            if (l0 > support * double(cfg.maxStretch) * (1.0 + kRound)) { std::printf("row %zu: |axis0| = %g above support * maxStretch\n", i, l0); return 7; }
            if (l0 / l2 > double(cfg.maxRatio) * (1.0 + kRound)) { std::printf("row %zu: |axis0| / |axis2| = %g above maxRatio\n", i, l0 / l2); return 8; }
            ratioSum += l2 / l0;
        }
        const SphAnisoInfo held = fluid.AnisoInfo();
        if (rows.size() != size_t(info.rows) || sparse != info.numSparse || clamped != info.numClamped || maxCount != info.maxCount ||
            maxReach != info.maxReach || held.rows != info.rows || held.numSparse != info.numSparse || held.numClamped != info.numClamped ||
            held.maxCount != info.maxCount || held.maxReach != info.maxReach || info.kind != 1) {
            std::printf("the info does not describe the rows\n");
            return 9;
        }
        SphSurface iso, aniso;
        if (!fluid.ExtractSurface(origin, Vec3(s, s, s), dims, SPH_FIELD_FRACTION, 0.5f, iso)) {
            std::printf("ExtractSurface failed: %s\n", fluid.LastError().c_str());
            return 10;
        }
        if (!fluid.ExtractAnisoSurface(cfg, origin, Vec3(s, s, s), dims, 0.5f, aniso) || !fluid.DownloadSurface(verts, tris)) {
            std::printf("ExtractAnisoSurface failed: %s\n", fluid.LastError().c_str());
            return 11;
        }
        if (verts.size() != aniso.numVertices || tris.size() != size_t(aniso.numTriangles) * 3) { std::printf("DownloadSurface: wrong sizes\n"); return 12; }
        std::unordered_map<uint64_t, int> edges;
        edges.reserve(tris.size() * 2);
        for (size_t t = 0; t < tris.size(); t += 3)
            for (int e = 0; e < 3; ++e) {
                const uint32_t a = tris[t + e], b = tris[t + (e + 1) % 3];
                if (a >= verts.size() || b >= verts.size() || a == b) { std::printf("triangle %zu: bad indices\n", t / 3); return 13; }
                edges[(uint64_t(std::min(a, b)) << 32) | std::max(a, b)] += 1;
            }
        for (const auto& kv : edges)
            if (kv.second != 2) { std::printf("edge (%u, %u) lies in %d triangles\n", unsigned(kv.first >> 32), unsigned(kv.first & 0xffffffffu), kv.second); return 14; }
        std::printf("frame %d rows=%zu sparse=%llu clamped=%llu mean |axis2|/|axis0|=%.4f isotropic vertices=%u triangles=%u anisotropic vertices=%u triangles=%u\n",
                    frame, rows.size(), (unsigned long long)sparse, (unsigned long long)clamped, valid ? ratioSum / double(valid) : 0.0, iso.numVertices,
                    iso.numTriangles, aniso.numVertices, aniso.numTriangles);
    }
    std::printf("aniso_surface OK\n");
    return 0;
}
