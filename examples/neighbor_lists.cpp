// neighbor_lists.cpp -- the engine's neighbour relation as an output, through the C++ twin only: the default scene for some frames,
// after each frame the CSR lists of every particle at R = h with the particle itself (SPH_NEIGHBORS_SELF), and three checks on them:
// every entry is a particle id, the relation is symmetric, and the degree of particle i equals the `count` SamplePoints gives at its
// position (the same accept test over the same candidates).  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/neighbor_lists.cpp -L <pkg dir> -lsph_hip -o neighbor_lists
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    std::vector<int64_t> offsets;
    std::vector<int32_t> indices;
    std::vector<SPHParticle> records;
    std::vector<Vec4> probes;
    std::vector<SphSample> samples;
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphNeighborInfo info;
        if (!fluid.Neighbors(info, fluid.param_h, SPH_NEIGHBORS_SELF) || !fluid.DownloadNeighbors(offsets, indices)) {
            std::printf("Neighbors failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        const size_t rows = size_t(info.rows);
        std::printf("frame %d rows=%zu total=%llu mean degree=%.3f max degree=%u\n", frame, rows, (unsigned long long)info.total,
                    rows ? double(info.total) / double(rows) : 0.0, info.maxCount);
        if (offsets.size() != rows + 1 || offsets[0] != 0 || uint64_t(offsets[rows]) != info.total || indices.size() != info.total) {
            std::printf("the offsets do not describe %llu entries\n", (unsigned long long)info.total);
            return 4;
        }
        for (int32_t j : indices)
            if (j < 0 || size_t(j) >= rows) { std::printf("entry %d is out of range\n", j); return 4; }
        // symmetry: i is listed in the row of every j it lists (rows hold ascending (cell, id), so a linear search)
        for (size_t i = 0; i < rows; ++i)
            for (int64_t a = offsets[i]; a < offsets[i + 1]; ++a) {
                const size_t j = size_t(indices[size_t(a)]);
                const auto b = indices.begin() + offsets[j], e = indices.begin() + offsets[j + 1];
                if (std::find(b, e, int32_t(i)) == e) { std::printf("%zu lists %zu but not the other way round\n", i, j); return 5; }
            }
        // degree == the sampler's count at the particle's position
        if (!fluid.Download(records)) { std::printf("Download failed: %s\n", fluid.LastError().c_str()); return 3; }
        probes.clear();
        for (const SPHParticle& p : records) probes.push_back(Vec4(p.pos.x, p.pos.y, p.pos.z, 0.0f));
        if (!fluid.SamplePoints(probes, samples)) { std::printf("SamplePoints failed: %s\n", fluid.LastError().c_str()); return 3; }
        for (size_t i = 0; i < rows; ++i)
            if (uint64_t(offsets[i + 1] - offsets[i]) != samples[i].count) {
                std::printf("particle %zu: degree %lld, sampled count %u\n", i, (long long)(offsets[i + 1] - offsets[i]), samples[i].count);
                return 6;
            }
    }
    std::printf("neighbor_lists OK\n");
    return 0;
}
