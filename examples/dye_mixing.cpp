// dye_mixing.cpp -- the stirred tank with the reference's marble dye as a diffusing scalar, through the C++
// twin.  Channel 0 is seeded from padB of the records; every substep carries it with the particles and lets it diffuse between
// neighbours, 16 substeps per frame as ONE sph_dispatch_n call.  Per frame: the variance of the dye over the fluid and the mixing
// index 1 - var / var0, which is what a stirred tank is for.
//
// Two checks make the program exit non-zero:
//   * the fp64 sum of the dye may drift by rounding only.  Per substep and particle the fma chain of the exchange and its finish
//     round at most (pairs + 4) eps32 (|c| + s (cmax - cmin)), s being the diffusion number; pairs is at most 27 times the largest
//     cell count, which the statistics report (exit 8);
//   * while the reported diffusion number is <= 1, no value leaves the initial [min, max] by more than that rounding (exit 9).
//
//   g++ -std=c++17 -I include examples/dye_mixing.cpp -L <pkg dir> -lsph_hip -o dye_mixing
//   ./dye_mixing [frames] [particles] [omega]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 10;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const float omega = argc > 3 ? (float)std::atof(argv[3]) : 4.0f;
    const int substeps = 16;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.param_dyePattern = 1;
    fluid.ResetSimulation();                                               // respawn with the marble dye in padB
    if (!fluid.LastError().empty()) return 2;
    for (int i = 0; i < 30; ++i) fluid.DispatchCompute();                  // let the spawned block settle a little first
    SphObstacle paddle;
    sph_obstacle_default(&paddle);
    paddle.shape = SPH_OBSTACLE_BOX;
    paddle.size[0] = 3.0f; paddle.size[1] = 2.5f; paddle.size[2] = 0.4f;
    paddle.center[0] = fluid.param_boxCenter.x;
    paddle.center[1] = fluid.param_boxCenter.y - fluid.param_boxHalf.y + 3.0f;
    paddle.center[2] = fluid.param_boxCenter.z;
    paddle.omega[1] = omega;
    if (!fluid.SetObstacles({paddle})) return 3;
    const float dt = fluid.param_timeStep;

    // the dye, with the diffusivity that gives a diffusion number of about 0.4 on this state: the number is linear in D
    if (!fluid.SetScalars({}, 1, {1.0f, 0.0f})) return 4;
    fluid.DispatchCompute();
    uint64_t steps = 0;
    float number = 0.0f;
    if (!fluid.ScalarInfo(steps, number) || steps != 1 || !(number > 0.0f)) { std::printf("no diffusion number after a substep\n"); return 4; }
    const float D = 0.4f / number;
    if (!fluid.SetScalars({}, 1, {D, 0.0f})) return 4;                    // seeded again: the probe substep is forgotten

    std::vector<SphScalarMoments> m;
    if (!fluid.ScalarMoments(m) || m.size() != 1 || m[0].count == 0) return 5;
    const double sum0 = m[0].sum, var0 = SPHFluidGPU::ScalarVariance(m[0]);
    const double lo = m[0].min.value, hi = m[0].max.value, cmax = std::fmax(std::fabs(lo), std::fabs(hi));
    if (!(var0 > 0.0)) { std::printf("the dye is uniform: nothing to mix\n"); return 5; }
    std::printf("dye: %llu particles, D=%.6g, sum=%.9g, variance=%.6g, range [%.6g, %.6g]\n", (unsigned long long)m[0].count, (double)D, sum0, var0, lo, hi);
    double driftAllowed = 0.0, valueAllowed = 0.0;
    bool numberOk = true;
    for (int frame = 0; frame < frames; ++frame) {
        SphStatistics st;
        if (!fluid.Statistics(st)) return 6;
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 6; }
        if (!fluid.ScalarInfo(steps, number) || !fluid.ScalarMoments(m)) return 7;
        SphStatistics after;
        if (!fluid.Statistics(after)) return 6;
        numberOk = numberOk && number <= 1.0f;
        // (cell counts before and after the frame bound the pairs of its substeps only roughly: twice the larger one is allowed for)
        const double pairs = 27.0 * 2.0 * double(st.maxCellCount > after.maxCellCount ? st.maxCellCount : after.maxCellCount) + 4.0;
        const double perValue = pairs * std::ldexp(1.0, -23) * (cmax + std::fmax(double(number), 1.0) * (hi - lo));
        valueAllowed += double(substeps) * perValue;
        driftAllowed += double(substeps) * perValue * double(m[0].count);
        const double var = SPHFluidGPU::ScalarVariance(m[0]);
        std::printf("frame %d substeps=%llu number=%.4f sum=%.9g drift=%.3g allowed=%.3g variance=%.6g mixing_index=%.6f min=%.6g max=%.6g\n", frame,
                    (unsigned long long)steps, (double)number, m[0].sum, m[0].sum - sum0, driftAllowed, var, 1.0 - var / var0, (double)m[0].min.value,
                    (double)m[0].max.value);
        if (std::fabs(m[0].sum - sum0) > driftAllowed) { std::printf("the dye's sum drifted by %.6g\n", m[0].sum - sum0); return 8; }
        if (numberOk && (double(m[0].min.value) < lo - valueAllowed || double(m[0].max.value) > hi + valueAllowed)) {
            std::printf("a value left the initial range [%.9g, %.9g]: [%.9g, %.9g]\n", lo, hi, (double)m[0].min.value, (double)m[0].max.value);
            return 9;
        }
    }
    std::printf("dye_mixing OK\n");
    return 0;
}
