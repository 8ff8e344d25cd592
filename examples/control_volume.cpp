// control_volume.cpp -- flow gates through the C++ twin: the default scene after a wave impulse, a box of six
// gates with outward normals around the middle of the fluid (a control volume) and one unbounded plane at its mid height.  16 substeps
// per frame as ONE sph_dispatch_n call; the gates are booked inside it, on the device.  Per frame: the plane's net count and
// discharge, the box's net outflow, and the particle counts they must agree with.
//
// Three checks make the program exit non-zero:
//   * the plane's forward - backward differs from the change in the number of particles on its forward side, counted from a download
//     before and after with the same side function (exit 6): exact by construction;
//   * the box's net outflow differs from the loss of particles inside it, counted the same way (exit 7): a crossing within a rounding
//     of a box edge could in principle be booked twice or not at all, which no run of this scene has shown;
//   * a history row is not later than the one before it (exit 8).
//
//   g++ -std=c++17 -I include examples/control_volume.cpp -L <pkg dir> -lsph_hip -o control_volume
//   ./control_volume [frames] [particles]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

// The side of section 3r: dot3(p - center, cross(u, v)) in fp32, the dot product as fmaf(z, z, fmaf(y, y, x * x)).
static float gate_side(const SphGate& g, const SPHParticle& p) {
    const float N[3] = {g.u[1] * g.v[2] - g.u[2] * g.v[1], g.u[2] * g.v[0] - g.u[0] * g.v[2], g.u[0] * g.v[1] - g.u[1] * g.v[0]};
    const float dx = p.pos.x - g.center[0], dy = p.pos.y - g.center[1], dz = p.pos.z - g.center[2];
    return std::fmaf(dz, N[2], std::fmaf(dy, N[1], dx * N[0]));
}
static bool counted(const SPHParticle& p) { return p.isGhost == 0 && std::isfinite(p.pos.x) && std::isfinite(p.pos.y) && std::isfinite(p.pos.z); }

// Particles on the forward side of the plane, and particles behind all six faces of the box.
static void census(const std::vector<SPHParticle>& rec, const std::vector<SphGate>& gates, long long& above, long long& inside) {
    above = inside = 0;
    for (const SPHParticle& p : rec) {
        if (!counted(p)) continue;
        if (gate_side(gates[6], p) >= 0.0f) ++above;
        bool in = true;
        for (int f = 0; f < 6; ++f) in = in && gate_side(gates[f], p) < 0.0f;
        if (in) ++inside;
    }
}

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 10;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const int substeps = 16;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    for (int i = 0; i < 30; ++i) fluid.DispatchCompute();                  // let the spawned block settle a little first
    const float dt = fluid.param_timeStep;
    std::vector<SPHParticle> rec;
    if (!fluid.Download(rec) || rec.empty()) return 3;

    // the fluid's bounding box: the control volume is its middle half, the plane its mid height
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const SPHParticle& p : rec) {
        if (!counted(p)) continue;
        const float q[3] = {p.pos.x, p.pos.y, p.pos.z};
        for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], q[a]); hi[a] = std::fmax(hi[a], q[a]); }
    }
    float center[3], half[3];
    for (int a = 0; a < 3; ++a) { center[a] = 0.5f * (lo[a] + hi[a]); half[a] = 0.25f * (hi[a] - lo[a]); }
    std::vector<SphGate> gates = SPHFluidGPU::GateBox(center, half);
    const float ux[3] = {0.0f, 0.0f, 1.0f}, vx[3] = {1.0f, 0.0f, 0.0f};    // cross(z, x) = +y: forward is up
    gates.push_back(SPHFluidGPU::Gate(SPH_GATE_RECT, center, ux, vx, /*unbounded=*/true));
    if (!fluid.SetGates(gates, /*history=*/64, /*stride=*/4)) { std::printf("%s\n", fluid.LastError().c_str()); return 4; }
    std::vector<SphGate> back;
    if (!fluid.GetGates(back) || back.size() != 7) return 4;

    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    long long above0 = 0, inside0 = 0;
    census(rec, gates, above0, inside0);
    std::printf("control volume: centre (%.3f %.3f %.3f) half (%.3f %.3f %.3f), %lld particles inside, %lld above the plane\n", (double)center[0],
                (double)center[1], (double)center[2], (double)half[0], (double)half[1], (double)half[2], inside0, above0);
    const double volume = double(fluid.param_mass) / double(fluid.param_restDensity);
    std::vector<SphGateBooks> books;
    double time = 0.0;
    uint64_t booked = 0;
    for (int frame = 0; frame < frames; ++frame) {
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 5; }
        if (!fluid.GateBooks(books, time, booked) || books.size() != 7 || !fluid.Download(rec)) { std::printf("%s\n", fluid.LastError().c_str()); return 5; }
        long long above = 0, inside = 0, outflow = 0, crossings = 0;
        census(rec, gates, above, inside);
        for (int f = 0; f < 6; ++f) {
            outflow += (long long)books[f].forward - (long long)books[f].backward;
            crossings += (long long)(books[f].forward + books[f].backward);
        }
        const long long net = (long long)books[6].forward - (long long)books[6].backward;
        std::printf("frame %d substeps=%llu t=%.5f plane: +%llu -%llu net %lld (above %lld -> %lld) discharge %.6g, upward momentum flux sum %.6g | box: %lld crossings, "
                    "net outflow %lld (inside %lld -> %lld) discharge %.6g\n", frame, (unsigned long long)booked, time, (unsigned long long)books[6].forward,
                    (unsigned long long)books[6].backward, net, above0, above, time > 0.0 ? double(net) * volume / time : 0.0, books[6].vel[1], crossings,
                    outflow, inside0, inside, time > 0.0 ? double(outflow) * volume / time : 0.0);
        if (booked != uint64_t(frame + 1) * uint64_t(substeps)) { std::printf("the books counted %llu substeps\n", (unsigned long long)booked); return 5; }
        if (net != above - above0) { std::printf("the plane booked a net %lld, the count above it changed by %lld\n", net, above - above0); return 6; }
        if (outflow != inside0 - inside) { std::printf("the box booked a net outflow of %lld, it lost %lld particles\n", outflow, inside0 - inside); return 7; }
    }
    std::vector<SphGateBooks> rows;
    std::vector<double> times;
    uint32_t stored = 0;
    uint64_t first = 0;
    if (!fluid.GateHistory(rows, times, stored, first)) { std::printf("%s\n", fluid.LastError().c_str()); return 8; }
    const uint64_t taken = uint64_t(frames) * uint64_t(substeps) / 4;
    if (stored != (taken < 64 ? taken : 64) || first + stored != taken || rows.size() != size_t(stored) * 7) {
        std::printf("history: %u rows from %llu, expected %llu taken\n", stored, (unsigned long long)first, (unsigned long long)taken);
        return 8;
    }
    for (uint32_t i = 1; i < stored; ++i) {
        if (!(times[i] > times[i - 1])) { std::printf("history row %u at t=%.9g is not later than row %u at t=%.9g\n", i, times[i], i - 1, times[i - 1]); return 8; }
    }
    std::printf("hydrograph: %u rows from row %llu, t=%.5f .. %.5f\n", stored, (unsigned long long)first, stored ? times[0] : 0.0, stored ? times[stored - 1] : 0.0);
    std::printf("control_volume OK\n");
    return 0;
}
