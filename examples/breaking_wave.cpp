// breaking_wave.cpp -- spray, foam and bubbles through the C++ twin: the 50 000-particle default scene under ApplyWaveImpulse every
// frame, 16 fixed-dt substeps per frame as ONE sph_dispatch_n call; the secondary particles are spawned, classed, moved and removed
// inside every substep, on the device.  Per frame one line of class counts.  Exits non-zero if a record is not finite or lies outside
// the grid's box, if the alive count exceeds the capacity, or if alive != seeded + spawned - dropped - all deaths.
//
//   g++ -std=c++17 -I include examples/breaking_wave.cpp -L <pkg dir> -lsph_hip -o breaking_wave
//   ./breaking_wave [frames] [particles] [capacity]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 8;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const int substeps = 16;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    SphDiffuseConfig cfg = SPHFluidGPU::DiffuseConfig();
    if (argc > 3) cfg.capacity = (uint32_t)std::atol(argv[3]);
    if (!fluid.SetDiffuse(cfg)) return 3;
    std::vector<SphDiffuse> pool;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        if (sph_dispatch_n(fluid.Handle(), fluid.param_timeStep, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        SphDiffuseInfo info;
        SphGridInfo g;
        if (!fluid.DiffuseInfo(info) || !fluid.DownloadDiffuse(pool) || sph_grid_info(fluid.Handle(), &g) != SPH_OK) return 5;
        size_t kinds[3] = {0, 0, 0};
        for (const SphDiffuse& d : pool) {
            for (int a = 0; a < 3; ++a) {
                const float hi = g.gridMin[a] + (float)g.dims[a] * g.cellSize;
                if (!std::isfinite(d.pos[a])) { std::printf("frame %d: a record is not finite\n", frame); return 6; }
                if (d.pos[a] < g.gridMin[a] || d.pos[a] > hi) { std::printf("frame %d: a record lies outside the grid's box\n", frame); return 7; }
            }
            if (d.kind > 2u) { std::printf("frame %d: kind %u\n", frame, d.kind); return 8; }
            kinds[d.kind] += 1;
        }
        if (info.alive > info.capacity || pool.size() != info.alive) { std::printf("frame %d: %u alive of %u\n", frame, info.alive, info.capacity); return 9; }
        const uint64_t gone = info.dropped + info.diedLife + info.diedAge + info.leftBox + info.nonFinite;
        if ((uint64_t)info.alive + gone != info.seeded + info.spawned) { std::printf("frame %d: the books do not balance\n", frame); return 10; }
        std::printf("frame %d spray=%zu foam=%zu bubbles=%zu alive=%u spawned=%llu dropped=%llu died_life=%llu died_age=%llu left_box=%llu\n", frame,
                    kinds[0], kinds[1], kinds[2], info.alive, (unsigned long long)info.spawned, (unsigned long long)info.dropped,
                    (unsigned long long)info.diedLife, (unsigned long long)info.diedAge, (unsigned long long)info.leftBox);
    }
    std::printf("breaking_wave OK\n");
    return 0;
}
