// thermal_plume.cpp -- the default scene with a temperature channel that acts back on the fluid, through the
// C++ twin.  A heater on the tank floor and a cooled lid relax the temperature of the fluid inside them (SPH_SOURCE_RELAX), a heated
// sphere drifts through the tank with a source riding on it (body frame), the channel diffuses between neighbours (section 3h) and
// every substep kicks the fluid against gravity by beta (T - Tref): warm water rises.  16 substeps per frame as ONE sph_dispatch_n
// call; sources, buoyancy and the body all act inside it.  Per frame: the moments of the temperature and what each source injected.
//
// Two checks make the program exit non-zero:
//   * a record that is non-finite or has left the grid (the statistics call; exit 7);
//   * the heat balance: with the decay at 0 the fp64 sum of the temperature may differ from the initial sum plus the sources' books
//     by rounding only (exit 8).  Allowed: per substep and particle the diffusion's fma chain and finish round at most
//     (pairs + 4) eps32 (|T| + s (Tmax - Tmin)) (s the diffusion number, pairs at most 27 times the largest cell count); the books are
//     fp64 sums of H exactly defined terms of at most (Tmax - Tmin), good to 2 (H - 1) 2^-53 H (Tmax - Tmin); the two moment sums are
//     fp64 sums of n values of at most Tmax, good to n 2^-53 n Tmax each.  RELAX never leaves the interval between a value and its
//     target, so every temperature stays within [Tmin, Tmax] of the targets up to the diffusion's own rounding.
//
//   g++ -std=c++17 -I include examples/thermal_plume.cpp -L <pkg dir> -lsph_hip -o thermal_plume
//   ./thermal_plume [frames] [particles]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 10;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const int substeps = 16;
    const float tCold = 0.0f, tHot = 1.0f, tBody = 2.0f;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    for (int i = 0; i < 30; ++i) fluid.DispatchCompute();                  // let the spawned block settle a little first
    const float dt = fluid.param_timeStep;
    const Vec3 c = fluid.param_boxCenter, half = fluid.param_boxHalf;
    const float floorY = c.y - half.y;

    // the heated sphere, drifting along x
    SphObstacle ball;
    sph_obstacle_default(&ball);
    ball.size[0] = 1.0f;
    ball.center[0] = c.x - 2.0f; ball.center[1] = floorY + 1.0f; ball.center[2] = c.z;
    ball.vel[0] = 1.5f;
    if (!fluid.SetObstacles({ball})) return 3;

    // the temperature: 0 everywhere, with the diffusivity that gives a diffusion number of about 0.4 on this state
    const std::vector<float> cold(sph_num_particles(fluid.Handle()), tCold);
    if (!fluid.SetScalars(cold, 1, {1.0f, 0.0f})) return 4;
    fluid.DispatchCompute();
    uint64_t steps = 0;
    float number = 0.0f;
    if (!fluid.ScalarInfo(steps, number) || steps != 1 || !(number > 0.0f)) { std::printf("no diffusion number after a substep\n"); return 4; }
    const float D = 0.4f / number;
    if (!fluid.SetScalars(cold, 1, {D, 0.0f})) return 4;                  // decay 0: the heat balance below is exact up to rounding

    SphScalarSource heater, lid, glow;
    sph_scalar_source_default(&heater);
    heater.shape = SPH_SOURCE_BOX; heater.mode = SPH_SOURCE_RELAX; heater.rate = 30.0f; heater.target = tHot;
    heater.center[0] = c.x; heater.center[1] = floorY + 0.4f; heater.center[2] = c.z;
    heater.size[0] = 0.5f * half.x; heater.size[1] = 0.5f; heater.size[2] = 0.5f * half.z;
    lid = heater;
    lid.target = tCold; lid.rate = 10.0f;
    lid.center[1] = floorY + 5.0f + half.y;                                // everything above 5 units over the floor
    lid.size[0] = half.x; lid.size[1] = half.y; lid.size[2] = half.z;
    sph_scalar_source_default(&glow);
    glow.mode = SPH_SOURCE_RELAX; glow.rate = 50.0f; glow.target = tBody;
    glow.body = 0;                                                         // rides on the sphere: centre 0 in its frame
    glow.size[0] = 1.6f;
    if (!fluid.SetScalarSources({heater, lid, glow})) { std::printf("%s\n", fluid.LastError().c_str()); return 5; }
    if (!fluid.SetScalarBuoyancy({0.5f}, {tCold})) { std::printf("%s\n", fluid.LastError().c_str()); return 5; }

    std::vector<SphScalarMoments> m;
    if (!fluid.ScalarMoments(m) || m.size() != 1 || m[0].count == 0) return 6;
    const double sum0 = m[0].sum, count = double(m[0].count);
    const double lo = tCold, hi = tBody, tmax = std::fmax(std::fabs(lo), std::fabs(hi));
    std::printf("temperature: %llu particles, D=%.6g, sum=%.9g\n", (unsigned long long)m[0].count, (double)D, sum0);
    double allowed = 0.0;
    std::vector<double> sums;
    std::vector<uint64_t> hits;
    double time = 0.0;
    uint64_t booked = 0;
    for (int frame = 0; frame < frames; ++frame) {
        SphStatistics st;
        if (!fluid.Statistics(st)) return 6;
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 6; }
        SphStatistics after;
        if (!fluid.ScalarInfo(steps, number) || !fluid.ScalarMoments(m) || !fluid.Statistics(after)) return 6;
        if (!fluid.ScalarInjected(sums, hits, time, booked) || sums.size() != 3) { std::printf("%s\n", fluid.LastError().c_str()); return 6; }
        if (after.numNonFinite || after.numEscaped) {
            std::printf("frame %d: %llu non-finite records, %llu escaped\n", frame, (unsigned long long)after.numNonFinite, (unsigned long long)after.numEscaped);
            return 7;
        }
        const double injected = sums[0] + sums[1] + sums[2], H = double(hits[0] + hits[1] + hits[2]);
        // (cell counts before and after the frame bound the pairs of its substeps only roughly: twice the larger one is allowed for)
        const double pairs = 27.0 * 2.0 * double(st.maxCellCount > after.maxCellCount ? st.maxCellCount : after.maxCellCount) + 4.0;
        allowed += double(substeps) * pairs * std::ldexp(1.0, -23) * (tmax + std::fmax(double(number), 1.0) * (hi - lo)) * count;
        const double books = 2.0 * H * std::ldexp(1.0, -53) * H * (hi - lo) + 2.0 * count * std::ldexp(1.0, -53) * count * tmax;
        const double balance = m[0].sum - (sum0 + injected);
        std::printf("frame %d substeps=%llu number=%.4f mean=%.6f min=%.6g max=%.6g sum=%.9g injected=%.9g (heater %.6g / %llu, lid %.6g / %llu, sphere %.6g / %llu) "
                    "balance=%.3g allowed=%.3g\n", frame, (unsigned long long)booked, (double)number, m[0].sum / count, (double)m[0].min.value,
                    (double)m[0].max.value, m[0].sum, injected, sums[0], (unsigned long long)hits[0], sums[1], (unsigned long long)hits[1], sums[2],
                    (unsigned long long)hits[2], balance, allowed + books);
        if (!(std::fabs(balance) <= allowed + books)) { std::printf("the heat balance is off by %.6g\n", balance); return 8; }
        if (booked != uint64_t(frame + 1) * uint64_t(substeps)) { std::printf("the books counted %llu substeps\n", (unsigned long long)booked); return 9; }
    }
    if (!(sums[0] > 0.0) || hits[0] == 0 || hits[2] == 0) { std::printf("the heater or the sphere never touched the fluid\n"); return 10; }
    std::printf("thermal_plume OK\n");
    return 0;
}
