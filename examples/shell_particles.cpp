// shell_particles.cpp -- the free-surface shell of the fluid, through the C++ twin only: the default scene gets a wave impulse, then
// once per frame the shell of the particles at R = h.  Prints the size of the shell, its share of all particles, the number of
// isolated particles and the mean and the largest crest measure over the shell (what a renderer draws, and where a spray model would
// spawn), and checks the result: ids are particle ids and ascend, ids are exactly the flagged rows, a shell normal that is not zero
// has unit length, a row outside the shell has no crest, and the counts are those of ShellInfo.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/shell_particles.cpp -L <pkg dir> -lsph_hip -o shell_particles
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    std::vector<SphShell> rows;
    std::vector<int32_t> ids;
    const SphShellConfig cfg = SPHFluidGPU::ShellConfig();
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphShellInfo info;
        if (!fluid.Shell(info, cfg) || !fluid.DownloadShell(rows, ids)) {
            std::printf("Shell failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        const SphShellInfo held = fluid.ShellInfo();
        if (rows.size() != size_t(info.rows) || ids.size() != size_t(info.numShell) || held.rows != info.rows || held.numShell != info.numShell ||
            held.numIsolated != info.numIsolated || held.maxCount != info.maxCount || info.kind != 1) {
            std::printf("the info does not describe the rows\n");
            return 4;
        }
        for (size_t s = 0; s < ids.size(); ++s) {
            if (ids[s] < 0 || size_t(ids[s]) >= rows.size()) { std::printf("ids[%zu] = %d is out of range\n", s, ids[s]); return 5; }
            if (s > 0 && ids[s] <= ids[s - 1]) { std::printf("ids do not ascend at %zu\n", s); return 5; }
            if (!(rows[size_t(ids[s])].flags & SPH_SHELL_MEMBER)) { std::printf("ids[%zu] = %d is not flagged\n", s, ids[s]); return 6; }
        }
        uint64_t shell = 0, isolated = 0;
        uint32_t maxCount = 0;
        double sum = 0.0, largest = 0.0;
        for (size_t i = 0; i < rows.size(); ++i) {
            const SphShell& r = rows[i];
            maxCount = std::max(maxCount, r.count);
            if (r.flags & SPH_SHELL_ISOLATED) isolated += 1;
            const double n2 = double(r.normal[0]) * r.normal[0] + double(r.normal[1]) * r.normal[1] + double(r.normal[2]) * r.normal[2];
            if (!(r.flags & SPH_SHELL_MEMBER)) {
                if (r.crest != 0.0f) { std::printf("row %zu is not in the shell and has crest %g\n", i, double(r.crest)); return 8; }
                continue;
            }
            shell += 1;
            if (n2 != 0.0 && std::fabs(n2 - 1.0) > 1e-5) { std::printf("row %zu: squared length of the normal %.9g\n", i, n2); return 7; }
            sum += r.crest;
            largest = std::max(largest, double(r.crest));
        }
        // (every id is flagged and ids ascend: as many flagged rows as ids means no flagged row is missing)
        if (shell != ids.size()) { std::printf("%llu flagged rows, %zu ids\n", (unsigned long long)shell, ids.size()); return 6; }
        if (shell != info.numShell || isolated != info.numIsolated || maxCount != info.maxCount) {
            std::printf("numShell / numIsolated / maxCount do not match the rows\n");
            return 9;
        }
        std::printf("frame %d rows=%zu shell=%llu (%.1f %%) isolated=%llu mean crest=%.4f max crest=%.4f\n", frame, rows.size(),
                    (unsigned long long)shell, rows.empty() ? 0.0 : 100.0 * double(shell) / double(rows.size()), (unsigned long long)isolated,
                    shell ? sum / double(shell) : 0.0, largest);
    }
    std::printf("shell_particles OK\n");
    return 0;
}
