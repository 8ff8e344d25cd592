// crest_spray.cpp -- spray born at wave crests through the C++ twin: the 50 000-particle default scene under ApplyWaveImpulse every
// frame, 16 fixed-dt substeps per frame as ONE sph_dispatch_n call, with the pool's foam term off (rate 0 in SphDiffuseConfig) and its
// crest term on: every child comes from a free-surface particle whose surface is sharply convex and moves along its own normal, found
// by a shell pass inside the substep, on the device.  Per frame one line: acting substeps, shell size, crest-born, alive by class.
// Exits non-zero if the books do not balance, if a record's parent is no particle, or if crest-born exceeds spawned.
//
//   g++ -std=c++17 -I include examples/crest_spray.cpp -L <pkg dir> -lsph_hip -o crest_spray
//   ./crest_spray [frames] [particles] [every]
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
    cfg.rate = 0.0f;                                                   // the foam term bears nobody
    if (!fluid.SetDiffuse(cfg)) return 3;
    SphDiffuseCrest crest = SPHFluidGPU::DiffuseCrest();
    if (argc > 3) crest.every = (uint32_t)std::atol(argv[3]);
    if (!fluid.SetDiffuseCrest(crest)) { std::printf("SetDiffuseCrest failed: %s\n", fluid.LastError().c_str()); return 3; }
    std::vector<SphDiffuse> pool;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        if (sph_dispatch_n(fluid.Handle(), fluid.param_timeStep, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        SphDiffuseInfo info;
        SphDiffuseCrestInfo books;
        if (!fluid.DiffuseInfo(info) || !fluid.DiffuseCrestInfo(books) || !fluid.DownloadDiffuse(pool)) return 5;
        size_t kinds[3] = {0, 0, 0};
        for (const SphDiffuse& d : pool) {
            if (d.parent >= n) { std::printf("frame %d: parent %u of %zu particles\n", frame, d.parent, n); return 6; }
            if (d.kind > 2u) { std::printf("frame %d: kind %u\n", frame, d.kind); return 7; }
            kinds[d.kind] += 1;
        }
        const uint64_t gone = info.dropped + info.diedLife + info.diedAge + info.leftBox + info.nonFinite;
        if (pool.size() != info.alive || (uint64_t)info.alive + gone != info.seeded + info.spawned) { std::printf("frame %d: the books do not balance\n", frame); return 8; }
        if (books.crestSpawned > info.spawned) { std::printf("frame %d: %llu crest-born of %llu spawned\n", frame, (unsigned long long)books.crestSpawned, (unsigned long long)info.spawned); return 9; }
        std::printf("frame %d acting=%llu shell=%u crest_born=%llu spray=%zu foam=%zu bubbles=%zu alive=%u spawned=%llu dropped=%llu\n", frame,
                    (unsigned long long)books.acting, books.shellSize, (unsigned long long)books.crestSpawned, kinds[0], kinds[1], kinds[2], info.alive,
                    (unsigned long long)info.spawned, (unsigned long long)info.dropped);
    }
    std::printf("crest_spray OK\n");
    return 0;
}
