// wave_gauge.cpp -- wave gauges beside ApplyWaveImpulse, through the C++ twin only: a box scene, a wave impulse every frame,
// fixed-dt substeps, and after each frame the water level at a few (x, z) points from SamplePoints along vertical lines
// (the rule of SPHFluidGPU.water_level in engine.py: from the top, the first height where `fraction` >= 0.5, interpolated
// linearly against the sample above it; NaN where no sample reaches it).
//
//   g++ -std=c++17 -I include examples/wave_gauge.cpp -L <pkg dir> -lsph_hip -o wave_gauge
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 12;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    const float h = fluid.param_h;
    const float gx[3] = {-3.0f, 0.0f, 3.0f}, gz[3] = {0.0f, 1.5f, -2.0f};
    const float yTop = fluid.param_boxCenter.y + fluid.param_boxHalf.y, yBot = fluid.param_boxCenter.y - fluid.param_boxHalf.y;
    const float dy = 0.125f * h;
    const int rows = int((yTop - yBot) / dy) + 1;
    std::vector<Vec4> probes;
    for (int g = 0; g < 3; ++g)
        for (int k = 0; k < rows; ++k) probes.push_back(Vec4(gx[g], yTop - float(k) * dy, gz[g], 0.0f));
    std::vector<SphSample> out;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        if (!fluid.SamplePoints(probes, out)) { std::printf("SamplePoints failed: %s\n", fluid.LastError().c_str()); return 3; }
        std::printf("frame %d", frame);
        for (int g = 0; g < 3; ++g) {
            float level = NAN;
            for (int k = 0; k < rows; ++k) {
                const float f = out[size_t(g) * rows + k].fraction;
                if (f < 0.5f) continue;
                const float y = probes[size_t(g) * rows + k].y;
                if (k == 0) { level = y; break; }
                const float fAbove = out[size_t(g) * rows + k - 1].fraction;
                level = y + dy * (f - 0.5f) / (f - fAbove);
                break;
            }
            std::printf(" gauge%d=%.4f", g, level);
        }
        std::printf("\n");
    }
    std::printf("wave_gauge OK\n");
    return 0;
}
