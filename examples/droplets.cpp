// droplets.cpp -- which particles hang together, through the C++ twin only: the default scene with a wave impulse, after each frame the
// connected bodies of the fluid (SPH_COMPONENTS_FLUID_ONLY) at R = h, one line per frame (bodies, the largest body, bodies of fewer than
// 64 particles), and four checks on the result: the counts of the table add up to the labelled records, every label is in range, the root
// of a body is its own root, and every member lies inside its body's box.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/droplets.cpp -L <pkg dir> -lsph_hip -o droplets
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    std::vector<int32_t> labels, roots;
    std::vector<SphComponent> table;
    std::vector<SPHParticle> records;
    for (int frame = 0; frame < frames; ++frame) {
        if (frame == 1) fluid.ApplyWaveImpulse(60.0f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphComponentInfo info;
        if (!fluid.Components(info, fluid.param_h, SPH_COMPONENTS_FLUID_ONLY) || !fluid.DownloadComponents(labels, roots, table) || !fluid.Download(records)) {
            std::printf("Components failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        size_t small = 0, labelled = 0;
        uint64_t members = 0;
        for (const SphComponent& c : table) { small += c.count < 64u ? 1u : 0u; members += c.count; }
        std::printf("frame %d bodies=%llu largest=%llu (root %u) under64=%zu rounds=%u\n", frame, (unsigned long long)info.numComponents,
                    (unsigned long long)info.largestCount, info.largestRoot, small, info.rounds);
        if (labels.size() != records.size() || roots.size() != records.size() || table.size() != info.numComponents) return 4;
        for (size_t i = 0; i < labels.size(); ++i) {
            const int32_t l = labels[i];
            if (l == -1 && roots[i] == -1 && records[i].isGhost != 0) continue;                  // left out: a ghost record
            if (l < 0 || size_t(l) >= table.size()) { std::printf("label %d of particle %zu is out of range\n", l, i); return 5; }
            labelled += 1;
            const SphComponent& c = table[size_t(l)];
            if (roots[i] != int32_t(c.root)) { std::printf("particle %zu: root %d, its body's %u\n", i, roots[i], c.root); return 6; }
            if (c.flags & SPH_COMPONENT_NONFINITE) continue;
            const float x[3] = {records[i].pos.x, records[i].pos.y, records[i].pos.z};
            for (int a = 0; a < 3; ++a)
                if (!(x[a] >= c.bbMin[a] && x[a] <= c.bbMax[a])) { std::printf("particle %zu lies outside the box of body %d\n", i, l); return 7; }
        }
        if (members != labelled || labelled + info.numExcluded != records.size()) {
            std::printf("the table counts %llu members, %zu records are labelled\n", (unsigned long long)members, labelled);
            return 8;
        }
        for (const SphComponent& c : table)
            if (c.root >= roots.size() || roots[c.root] != int32_t(c.root)) { std::printf("root %u is not its own root\n", c.root); return 9; }
    }
    std::printf("droplets OK\n");
    return 0;
}
