// neighbor_mean.cpp -- fused neighbourhood reductions of a caller's data, through the C++ twin only: the default scene gets a wave
// impulse, then once per frame the mean velocity difference to the neighbours within h (MEAN of v_j - v_i) and the first-moment sums of
// the velocity (SUM with MOMENTS: sum v_j and sum d_a v_j, d = x_j - x_i, the raw sums a velocity gradient is assembled from).  Prints
// the largest |mean dv| and the mean degree, and checks: every count is the degree of the neighbour lists at the same radius, an empty
// row is all zero, and plane 0 of the MOMENTS call is the plain SUM call byte for byte.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/neighbor_mean.cpp -L <pkg dir> -lsph_hip -o neighbor_mean
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    const int C = 3;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    std::vector<SPHParticle> now;
    std::vector<float> vel, meanDv, moments, sum;
    std::vector<uint32_t> counts, countsM;
    std::vector<int64_t> offsets;
    std::vector<int32_t> none;
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        if (!fluid.Download(now)) return 3;
        const size_t rows = now.size();
        vel.resize(rows * C);
        for (size_t i = 0; i < rows; ++i) { vel[i * C] = now[i].vel.x; vel[i * C + 1] = now[i].vel.y; vel[i * C + 2] = now[i].vel.z; }
        SphAggregateConfig cfg = fluid.AggregateConfig();                        // radius = param_h
        cfg.channels = C;
        SphAggregateInfo info;
        SphAggregateConfig mean = cfg;
        mean.op = SPH_AGGREGATE_MEAN;
        mean.flags = SPH_AGGREGATE_DELTA;
        SphAggregateConfig mom = cfg;
        mom.flags = SPH_AGGREGATE_MOMENTS;
        if (!fluid.Aggregate(info, mean, vel, meanDv, &counts) || !fluid.Aggregate(info, mom, vel, moments, &countsM) || !fluid.Aggregate(info, cfg, vel, sum)) {
            std::printf("Aggregate failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        if (meanDv.size() != rows * C || moments.size() != rows * 4 * C || sum.size() != rows * C || counts.size() != rows) {
            std::printf("the results do not have the shapes asked for\n");
            return 4;
        }
        SphNeighborInfo nb;
        if (!fluid.Neighbors(nb, fluid.param_h, SPH_NEIGHBORS_COUNT_ONLY) || !fluid.DownloadNeighbors(offsets, none)) {
            std::printf("Neighbors failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        double largest = 0.0;
        uint64_t total = 0;
        for (size_t i = 0; i < rows; ++i) {
            const int64_t degree = offsets[i + 1] - offsets[i];
            if (int64_t(counts[i]) != degree || countsM[i] != counts[i]) {
                std::printf("particle %zu: %u candidates reduced, degree %lld\n", i, counts[i], (long long)degree);
                return 5;
            }
            total += counts[i];
            if (std::memcmp(&moments[i * 4 * C], &sum[i * C], C * sizeof(float)) != 0) {
                std::printf("particle %zu: plane 0 of the MOMENTS call is not the SUM call\n", i);
                return 6;
            }
            if (counts[i] == 0) {
                bool zero = true;
                for (int c = 0; c < C; ++c) zero = zero && meanDv[i * C + c] == 0.0f && sum[i * C + c] == 0.0f;
                for (int c = 0; c < 4 * C; ++c) zero = zero && moments[i * 4 * C + c] == 0.0f;
                if (!zero) { std::printf("particle %zu: an empty row is not all zero\n", i); return 7; }
            }
            const double x = meanDv[i * C], y = meanDv[i * C + 1], z = meanDv[i * C + 2];
            largest = std::max(largest, std::sqrt(x * x + y * y + z * z));
        }
        std::printf("frame %d rows=%zu mean degree=%.3f max |mean dv|=%.5f\n", frame, rows, rows ? double(total) / double(rows) : 0.0, largest);
    }
    std::printf("neighbor_mean OK\n");
    return 0;
}
