// column_depth.cpp -- the water's column depth under a wave, through the C++ twin only: the default scene gets a wave impulse, then once
// per frame a 64 x 64 sheet of parallel rays goes straight down from above the grid's box through ALL the particles (spheres of radius
// h / 4): per ray the number of spheres crossed, where the ray enters the first and leaves the last, and the summed thickness -- also
// under an overhanging crest, where a first-hit cast sees the top sheet only.  Prints the crossed rays, the mean and the largest
// thickness and the largest count, and checks the rows: ids are particle ids, a ray that crosses nothing is (+inf, -inf, -1, -1, 0),
// tEnter <= tExit, length <= count * 2^24, the counts are RaySpansInfo's, and -- these rays start outside every sphere and have
// tmax = +inf -- tEnter / idEnter are the t / id of CastRays bit for bit.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/column_depth.cpp -L <pkg dir> -lsph_hip -o column_depth
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    const int side = 64;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    fluid.ComputeGridExtents();
    const float r = 0.25f * fluid.param_h;
    const float x0 = fluid.gridMinV.x, z0 = fluid.gridMinV.z, top = fluid.gridMinV.y + fluid.cellSize * float(fluid.gridSizeY) + 1.0f;
    const float ex = fluid.cellSize * float(fluid.gridSizeX), ez = fluid.cellSize * float(fluid.gridSizeZ);
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> rays;
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const float ray[8] = {x0 + ex * (float(i) + 0.5f) / float(side), top, z0 + ez * (float(j) + 0.5f) / float(side), 0.0f, 0.0f, -1.0f, 0.0f, inf};
            rays.insert(rays.end(), ray, ray + 8);
        }
    std::vector<SphRaySpan> rows;
    std::vector<SphRayHit> hits;
    std::vector<SPHParticle> now;
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphRaySpansInfo info;
        SphRaysInfo cast;
        if (!fluid.SpanRays(rays, info, r) || !fluid.DownloadRaySpans(rows) || !fluid.CastRays(rays, cast, r) || !fluid.DownloadRayHits(hits) ||
            !fluid.Download(now)) {
            std::printf("SpanRays / CastRays failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        const size_t count = now.size();
        if (info.rays != uint64_t(side * side) || rows.size() != size_t(side * side) || hits.size() != rows.size() || info.voidRays != 0) {
            std::printf("the info does not describe the rows\n");
            return 4;
        }
        uint64_t crossed = 0, total = 0;
        uint32_t maxCount = 0;
        double sum = 0.0, largest = 0.0;
        for (size_t i = 0; i < rows.size(); ++i) {
            const SphRaySpan& s = rows[i];
            if (s.flags != 0) { std::printf("ray %zu: flags %u\n", i, s.flags); return 5; }
            if (s.count == 0) {
                if (!(s.tEnter == inf && s.tExit == -inf && s.idEnter == -1 && s.idExit == -1 && s.length == 0)) {
                    std::printf("ray %zu: nothing crossed is not (+inf, -inf, -1, -1, 0)\n", i);
                    return 6;
                }
            } else {
                if (s.idEnter < 0 || size_t(s.idEnter) >= count || s.idExit < 0 || size_t(s.idExit) >= count) {
                    std::printf("ray %zu: ids %d, %d out of range\n", i, s.idEnter, s.idExit);
                    return 7;
                }
                if (!(s.tEnter <= s.tExit)) { std::printf("ray %zu: tEnter %g > tExit %g\n", i, double(s.tEnter), double(s.tExit)); return 8; }
                if (s.length > (uint64_t(s.count) << 24)) { std::printf("ray %zu: length above count diameters\n", i); return 9; }
                crossed += 1;
            }
            // the first entry is what the cast finds: the same t bit for bit and the same id (a miss there is t = +inf, id = -1 too)
            if (std::memcmp(&s.tEnter, &hits[i].t, sizeof(float)) != 0 || s.idEnter != hits[i].id) {
                std::printf("ray %zu: tEnter %g id %d against the cast's t %g id %d\n", i, double(s.tEnter), s.idEnter, double(hits[i].t), hits[i].id);
                return 10;
            }
            total += s.count;
            maxCount = std::max(maxCount, s.count);
            const double thick = double(s.length) * 2.0 * double(r) * std::ldexp(1.0, -24);
            sum += thick;
            largest = std::max(largest, thick);
        }
        if (crossed != info.crossed || total != info.total || maxCount != info.maxCount || cast.hits != info.crossed) {
            std::printf("crossed %llu total %llu maxCount %u: RaySpansInfo has %llu, %llu, %u, the cast hit %llu\n", (unsigned long long)crossed,
                        (unsigned long long)total, maxCount, (unsigned long long)info.crossed, (unsigned long long)info.total, info.maxCount,
                        (unsigned long long)cast.hits);
            return 11;
        }
        std::printf("frame %d rays=%d crossed=%llu thickness mean=%.5f max=%.5f largest count=%u\n", frame, side * side, (unsigned long long)crossed,
                    crossed ? sum / double(crossed) : 0.0, largest, maxCount);
    }
    std::printf("column_depth OK\n");
    return 0;
}
