// knn_spacing.cpp -- the local particle spacing from the k nearest neighbours, through the C++ twin only: the default scene gets a
// wave impulse, then once per frame the 8 nearest neighbours of every particle within 2h.  Prints the number of full rows and the mean
// and the largest distance to the 8th neighbour over them (the quantity an adaptive smoothing length is set from), and checks the
// rows: every entry is a particle id, a row ascends in (dist2, id), padding is (-1, +inf), and counts[i] = min(8, degree_i) with the
// degrees of the neighbour lists at the same radius.  Exits non-zero if one of them fails.
//
//   g++ -std=c++17 -I include examples/knn_spacing.cpp -L <pkg dir> -lsph_hip -o knn_spacing
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    const int k = 8;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    std::vector<int32_t> indices;
    std::vector<float> dist2;
    std::vector<uint32_t> counts;
    std::vector<int64_t> offsets;
    std::vector<int32_t> none;
    const float R = 2.0f * fluid.param_h;
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphKnnInfo info;
        if (!fluid.Knn(info, k, R) || !fluid.DownloadKnn(indices, dist2, counts)) {
            std::printf("Knn failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        const size_t rows = size_t(info.rows);
        if (info.k != k || counts.size() != rows || indices.size() != rows * k || dist2.size() != rows * k) {
            std::printf("the info does not describe the rows\n");
            return 4;
        }
        double sum = 0.0, largest = 0.0;
        uint64_t full = 0, total = 0;
        for (size_t i = 0; i < rows; ++i) {
            const uint32_t c = counts[i];
            if (c > uint32_t(k)) { std::printf("row %zu has %u entries\n", i, c); return 4; }
            for (uint32_t s = 0; s < uint32_t(k); ++s) {
                const int32_t j = indices[i * k + s];
                const float d = dist2[i * k + s];
                if (s >= c) {
                    if (j != -1 || !(std::isinf(d) && d > 0.0f)) { std::printf("row %zu: entry %u is not padding\n", i, s); return 5; }
                    continue;
                }
                if (j < 0 || size_t(j) >= rows || size_t(j) == i) { std::printf("row %zu: entry %d is out of range\n", i, j); return 4; }
                if (s > 0) {
                    const int32_t jp = indices[i * k + s - 1];
                    const float dp = dist2[i * k + s - 1];
                    if (!(dp < d || (dp == d && jp < j))) { std::printf("row %zu is not ascending at entry %u\n", i, s); return 6; }
                }
            }
            total += c;
            if (c == uint32_t(k)) {
                const double d8 = std::sqrt(double(dist2[i * k + k - 1]));
                sum += d8;
                largest = std::max(largest, d8);
                full += 1;
            }
        }
        if (full != info.rowsFull || total != info.total) { std::printf("rowsFull / total do not match the rows\n"); return 7; }
        // counts[i] == min(k, degree_i) with the degrees of the neighbour lists at the same radius
        SphNeighborInfo nb;
        if (!fluid.Neighbors(nb, R, SPH_NEIGHBORS_COUNT_ONLY) || !fluid.DownloadNeighbors(offsets, none)) {
            std::printf("Neighbors failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        for (size_t i = 0; i < rows; ++i) {
            const int64_t degree = offsets[i + 1] - offsets[i];
            if (int64_t(counts[i]) != std::min<int64_t>(k, degree)) {
                std::printf("particle %zu: %u entries, degree %lld\n", i, counts[i], (long long)degree);
                return 8;
            }
        }
        std::printf("frame %d rows=%zu rowsFull=%llu mean d8=%.5f max d8=%.5f (2h = %.5f)\n", frame, rows, (unsigned long long)info.rowsFull,
                    full ? sum / double(full) : 0.0, largest, double(R));
    }
    std::printf("knn_spacing OK\n");
    return 0;
}
