// mean_flow.cpp -- field monitors through the C++ twin: the stirred tank (a box paddle spinning in the default
// scene), a spin-up, then ResetMonitor: the averaging starts from a developed flow.  Slot 0: eight gauge probes around the paddle with a
// ring of their raw samples; slot 1: a lattice of spacing h over the tank, sampled every 4th substep.  16 substeps per frame, 15 of them
// as ONE sph_dispatch_n call; the monitors run inside it, on the device.  Per frame: acting substeps, the wet share at the gauges, the
// largest mean speed and the largest turbulent kinetic energy on the lattice.
//
// The program exits non-zero if
//   * a row has wet > samples, or samples > the monitor's acting substeps (exit 6);
//   * a variance from MonitorField lies below -1e-9 * its second moment (exit 7).  A variance is second - mean^2 with
//     second = S2 / n and mean = S / n; exactly, second >= mean^2.  In fp64 (u = 2^-53) the running sum S2 of n non-negative terms is off
//     by at most (n - 1) u S2, S by at most (n - 1) u sum|x|, each division and the square add one u, and (sum|x| / n)^2 <= second, so
//     the computed difference lies above -(3 n + 6) u * second: cancellation only.  For n up to 3e6 samples that is above -1e-9 * second;
//     the final rounding to fp32 keeps the sign.
//   * a ring time does not ascend (exit 8);
//   * the ring's last sample of gauge 0 differs in a byte from SamplePoints taken before the dispatch that wrote it (exit 9).
//
//   g++ -std=c++17 -I include examples/mean_flow.cpp -L <pkg dir> -lsph_hip -o mean_flow
//   ./mean_flow [frames] [particles] [omega]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    for (int i = 0; i < 30; ++i) fluid.DispatchCompute();                  // let the spawned block settle a little first
    SphObstacle paddle;
    sph_obstacle_default(&paddle);
    paddle.shape = SPH_OBSTACLE_BOX;
    paddle.size[0] = 3.0f; paddle.size[1] = 2.5f; paddle.size[2] = 0.4f;   // a blade 6 wide, 5 high, 0.8 thick
    paddle.center[0] = fluid.param_boxCenter.x;
    paddle.center[1] = fluid.param_boxCenter.y - fluid.param_boxHalf.y + 3.0f;
    paddle.center[2] = fluid.param_boxCenter.z;
    paddle.omega[1] = omega;
    if (!fluid.SetObstacles({paddle})) return 3;
    const float dt = fluid.param_timeStep, h = fluid.param_h;

    // slot 0: eight gauges on a circle of 0.6 box half-widths around the paddle's axis, one unit above the floor, with a ring
    std::vector<Vec4> gauges;
    for (int g = 0; g < 8; ++g) {
        const float a = 0.78539816f * float(g);
        gauges.push_back(Vec4(fluid.param_boxCenter.x + 0.6f * fluid.param_boxHalf.x * std::cos(a), fluid.param_boxCenter.y - fluid.param_boxHalf.y + 1.0f,
                              fluid.param_boxCenter.z + 0.6f * fluid.param_boxHalf.z * std::sin(a), 0.0f));
    }
    SphMonitorConfig probeCfg = SPHFluidGPU::MonitorConfig();
    probeCfg.history = 64; probeCfg.stride = 1; probeCfg.ringPoints = 8;
    // slot 1: a lattice of spacing h over the tank, every 4th substep
    const Vec3 origin(fluid.param_boxCenter.x - fluid.param_boxHalf.x, fluid.param_boxCenter.y - fluid.param_boxHalf.y, fluid.param_boxCenter.z - fluid.param_boxHalf.z);
    const int dims[3] = {int(2.0f * fluid.param_boxHalf.x / h) + 1, int(2.0f * fluid.param_boxHalf.y / h) + 1, int(2.0f * fluid.param_boxHalf.z / h) + 1};
    SphMonitorConfig latticeCfg = SPHFluidGPU::MonitorConfig();
    latticeCfg.every = 4;
    if (!fluid.SetMonitor(0, gauges, probeCfg) || !fluid.SetMonitorLattice(1, origin, Vec3(h, h, h), dims, latticeCfg)) {
        std::printf("%s\n", fluid.LastError().c_str());
        return 4;
    }
    for (int i = 0; i < 2; ++i)                                            // the spin-up: the monitors run, their sums are thrown away below
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 5; }
    if (!fluid.ResetMonitor(0) || !fluid.ResetMonitor(1)) { std::printf("%s\n", fluid.LastError().c_str()); return 4; }
    std::printf("mean flow: %zu particles, paddle omega %.2f, 8 gauges, lattice %d x %d x %d at spacing %.3f\n", fluid.GetNumFluids(), (double)omega, dims[0], dims[1],
                dims[2], (double)h);

    std::vector<SphMonitorRow> probes, rows;
    std::vector<SphSample> before, ring;
    std::vector<double> times;
    std::vector<float> mx, my, mz, tke, varF, varP;
    for (int frame = 0; frame < frames; ++frame) {
        if (sph_dispatch_n(fluid.Handle(), dt, substeps - 1) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 5; }
        if (!fluid.SamplePoints(gauges, before)) { std::printf("%s\n", fluid.LastError().c_str()); return 5; }   // what the frame's last substep must record
        if (sph_dispatch(fluid.Handle(), dt) != SPH_OK) { std::printf("sph_dispatch failed: %s\n", sph_last_error()); return 5; }
        SphMonitorInfo info0, info1;
        if (!fluid.MonitorInfo(0, info0) || !fluid.MonitorInfo(1, info1) || !fluid.DownloadMonitor(0, probes) || !fluid.DownloadMonitor(1, rows)) {
            std::printf("%s\n", fluid.LastError().c_str());
            return 5;
        }
        const uint64_t done = uint64_t(frame + 1) * uint64_t(substeps);
        if (info0.substeps != done || info0.acting != done || info1.substeps != done || info1.acting != done / 4 || rows.size() != size_t(dims[0]) * dims[1] * dims[2]) {
            std::printf("the monitors counted %llu / %llu and %llu / %llu substeps\n", (unsigned long long)info0.substeps, (unsigned long long)info0.acting,
                        (unsigned long long)info1.substeps, (unsigned long long)info1.acting);
            return 5;
        }
        double wetShare = 0.0;
        for (const SphMonitorRow& r : probes) {
            if (r.wet > r.samples || r.samples > info0.acting) { std::printf("a gauge row has wet %llu, samples %llu of %llu acting\n", (unsigned long long)r.wet, (unsigned long long)r.samples, (unsigned long long)info0.acting); return 6; }
            wetShare += r.samples ? double(r.wet) / double(r.samples) / double(probes.size()) : 0.0;
        }
        for (const SphMonitorRow& r : rows)
            if (r.wet > r.samples || r.samples > info1.acting) { std::printf("a lattice row has wet %llu, samples %llu of %llu acting\n", (unsigned long long)r.wet, (unsigned long long)r.samples, (unsigned long long)info1.acting); return 6; }
        if (!fluid.MonitorField(1, SPH_MONITOR_MEAN_VEL_X, mx) || !fluid.MonitorField(1, SPH_MONITOR_MEAN_VEL_Y, my) || !fluid.MonitorField(1, SPH_MONITOR_MEAN_VEL_Z, mz) ||
            !fluid.MonitorField(1, SPH_MONITOR_TKE, tke) || !fluid.MonitorField(1, SPH_MONITOR_VAR_FRACTION, varF) || !fluid.MonitorField(1, SPH_MONITOR_VAR_PRESSURE, varP)) {
            std::printf("%s\n", fluid.LastError().c_str());
            return 5;
        }
        double speed = 0.0, energy = 0.0;
        for (size_t i = 0; i < rows.size(); ++i) {
            const SphMonitorRow& r = rows[i];
            const double secondF = r.samples ? r.sumFraction2 / double(r.samples) : 0.0, secondP = r.wet ? r.sumPressure2 / double(r.wet) : 0.0;
            const double secondV = r.wet ? 0.5 * (r.sumVelVel[0] + r.sumVelVel[1] + r.sumVelVel[2]) / double(r.wet) : 0.0;
            if (double(varF[i]) < -1e-9 * secondF || double(varP[i]) < -1e-9 * secondP || double(tke[i]) < -1e-9 * secondV) {
                std::printf("lattice point %zu: variances %g %g %g against second moments %g %g %g\n", i, (double)varF[i], (double)varP[i], (double)tke[i], secondF, secondP, secondV);
                return 7;
            }
            speed = std::fmax(speed, std::sqrt(double(mx[i]) * mx[i] + double(my[i]) * my[i] + double(mz[i]) * mz[i]));
            energy = std::fmax(energy, double(tke[i]));
        }
        uint32_t stored = 0;
        uint64_t first = 0;
        if (!fluid.MonitorHistory(0, ring, times, stored, first) || stored == 0 || first + stored != done || ring.size() != size_t(stored) * 8) {
            std::printf("history: %u rows from %llu after %llu acting substeps (%s)\n", stored, (unsigned long long)first, (unsigned long long)done, fluid.LastError().c_str());
            return 8;
        }
        for (uint32_t i = 1; i < stored; ++i)
            if (!(times[i] > times[i - 1])) { std::printf("ring row %u at t=%.9g is not later than row %u at t=%.9g\n", i, times[i], i - 1, times[i - 1]); return 8; }
        if (std::memcmp(&ring[size_t(stored - 1) * 8], &before[0], sizeof(SphSample)) != 0) {
            std::printf("the ring's last sample of gauge 0 (fraction %.9g) is not the sample taken before the dispatch (fraction %.9g)\n",
                        (double)ring[size_t(stored - 1) * 8].fraction, (double)before[0].fraction);
            return 9;
        }
        std::printf("frame %d acting=%llu/%llu t=%.5f wet share at the gauges %.3f, largest mean speed %.4f, largest TKE %.4f\n", frame, (unsigned long long)info0.acting,
                    (unsigned long long)info1.acting, info0.time, wetShare, speed, energy);
    }
    std::printf("mean_flow OK\n");
    return 0;
}
