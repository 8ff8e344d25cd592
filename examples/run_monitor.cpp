// run_monitor.cpp -- a headless run that watches itself: Scene0p's frame loop (ApplyWaveImpulse, 16 fixed-dt substeps) through the
// C++ twin, and after every frame one line of state statistics reduced on the GPU (no download): counted records, maximum speed,
// CFL number, kinetic energy, largest density over the rest density, members of the fullest cell.  The run ends with a non-zero
// status as soon as a non-finite or an escaped record appears, naming the lowest id among them.
//
//   g++ -std=c++17 -I include examples/run_monitor.cpp -L <pkg dir> -lsph_hip -o run_monitor
//   ./run_monitor [frames] [particles] [id to poison after frame 3]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 20;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const long poison = argc > 3 ? std::atol(argv[3]) : -1;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        for (int k = 0; k < 16; ++k) fluid.DispatchCompute(fluid.param_timeStep);
        if (frame == 3 && poison >= 0) {                               // what a diverging run looks like: one velocity becomes NaN
            std::vector<SPHParticle> host;
            if (!fluid.Download(host) || (size_t)poison >= host.size()) return 3;
            host[(size_t)poison].vel.y = std::numeric_limits<float>::quiet_NaN();
            if (sph_upload_particles(fluid.Handle(), reinterpret_cast<const SphParticle*>(host.data()), host.size()) != SPH_OK) return 3;
        }
        SphStatistics s;
        if (!fluid.Statistics(s)) { std::printf("Statistics failed: %s\n", fluid.LastError().c_str()); return 4; }
        std::printf("frame %d counted=%llu vmax=%.4f cfl=%.4f ekin=%.6e rhomax_over_rho0=%.4f largest_cell=%u\n", frame,
                    (unsigned long long)s.numCounted, s.maxSpeed, fluid.Cfl(s), fluid.KineticEnergy(s),
                    s.maxDensity.value / fluid.param_restDensity, s.maxCellCount);
        if (s.numNonFinite) { std::printf("non-finite record: %llu, first id %u\n", (unsigned long long)s.numNonFinite, s.firstNonFiniteId); return 10; }
        if (s.numEscaped) { std::printf("escaped record: %llu, first id %u\n", (unsigned long long)s.numEscaped, s.firstEscapedId); return 11; }
    }
    std::printf("run_monitor OK\n");
    return 0;
}
