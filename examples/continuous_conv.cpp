// continuous_conv.cpp -- the filter-grid basis sums of a continuous convolution through the C++ twin only: the default scene is stepped,
// the velocity (three channels) is expanded into the K^3 = 27 basis sums around every particle and around a coarse lattice of query
// points (AggregateBasis), and a tensor of that shape is taken back to the particles by the exact transposes (AggregateBasisAdjoint).
// The learned part of a layer would be one matrix product with the filters; here the filters are constant, so the planes of every row
// must add up to the plain neighbourhood sum.  Checks, each with an exit code of its own:
//   * every result has the bytes of the host twin of the same call (sph_aggregate_basis_host / _adjoint_host);
//   * partition of unity: sum_b A[i][b][c] equals Aggregate's SUM at the same weight within (k + 8) 2^-23 times the sum of |w v| (k
//     terms per accumulator on either side, three more roundings per coefficient, lo + hi = 1 to one rounding per axis).
// With a second argument the inputs and the four results are written to that file, for a comparison from outside.
//
//   g++ -std=c++17 -I include examples/continuous_conv.cpp -L <pkg dir> -lsph_hip -o continuous_conv
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

template <class T>
static bool put(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 20000;
    const int C = 3, K = 3, B = K * K * K;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    for (int s = 0; s < 4; ++s) fluid.DispatchCompute(fluid.param_timeStep);
    std::vector<SPHParticle> now;
    if (!fluid.Download(now)) return 3;
    const size_t rows = now.size();
    std::vector<float> vel(rows * C), speed(rows * C);
    for (size_t i = 0; i < rows; ++i) {
        vel[i * C] = now[i].vel.x; vel[i * C + 1] = now[i].vel.y; vel[i * C + 2] = now[i].vel.z;
        for (int c = 0; c < C; ++c) speed[i * C + c] = std::fabs(vel[i * C + c]);
    }
    fluid.ComputeGridExtents();
    const float spacing = 1.5f * fluid.param_h;
    const int dims[3] = {std::max(1, int(fluid.gridSizeX * fluid.cellSize / spacing) + 1), std::max(1, int(fluid.gridSizeY * fluid.cellSize / spacing) + 1),
                         std::max(1, int(fluid.gridSizeZ * fluid.cellSize / spacing) + 1)};
    const size_t m = size_t(dims[0]) * dims[1] * dims[2];
    std::vector<float> points(m * 4, 0.0f);
    for (size_t p = 0; p < m; ++p) {
        points[4 * p] = fluid.gridMinV.x + spacing * float(p % dims[0]);
        points[4 * p + 1] = fluid.gridMinV.y + spacing * float((p / dims[0]) % dims[1]);
        points[4 * p + 2] = fluid.gridMinV.z + spacing * float(p / (size_t(dims[0]) * dims[1]));
    }
    SphBasisConfig cfg = fluid.BasisConfig();                      // poly6, K = 4, R = h
    cfg.radius = 2.0f * fluid.param_h;
    cfg.size = K;
    cfg.channels = C;
    cfg.flags = SPH_AGGREGATE_SELF;
    SphBasisConfig qcfg = cfg;
    qcfg.flags = 0;                                                // (SELF applies to particle targets only)
    SphAggregateInfo info;
    std::vector<float> around, onLattice, back, backFromLattice;
    std::vector<uint32_t> counts;
    if (!fluid.AggregateBasis(info, cfg, vel, around, &counts) || !fluid.AggregateBasis(info, qcfg, vel, onLattice, nullptr, points.data(), m) ||
        !fluid.AggregateBasisAdjoint(info, cfg, around, back) || !fluid.AggregateBasisAdjoint(info, qcfg, onLattice, backFromLattice, points.data(), m)) {
        std::printf("a call failed: %s\n", fluid.LastError().c_str());
        return 3;
    }
    if (around.size() != rows * B * C || onLattice.size() != m * B * C || back.size() != rows * C || backFromLattice.size() != rows * C || info.planes != B) {
        std::printf("the results do not have the shapes asked for\n");
        return 4;
    }
    // the host twins of the four calls: the same bytes
    SphParams params;                                              // (what the calls above pushed)
    if (sph_get_params(fluid.Handle(), &params)) return 3;
    const SphParticle* rec = reinterpret_cast<const SphParticle*>(now.data());
    std::vector<float> hostAround(around.size()), hostLattice(onLattice.size()), hostBack(back.size()), hostBackLattice(backFromLattice.size());
    std::vector<uint32_t> hostCounts(rows);
    if (sph_aggregate_basis_host(rec, rows, &params, &cfg, nullptr, 0, vel.data(), hostAround.data(), hostCounts.data()) ||
        sph_aggregate_basis_host(rec, rows, &params, &qcfg, points.data(), m, vel.data(), hostLattice.data(), nullptr) ||
        sph_aggregate_basis_adjoint_host(rec, rows, &params, &cfg, nullptr, 0, around.data(), hostBack.data()) ||
        sph_aggregate_basis_adjoint_host(rec, rows, &params, &qcfg, points.data(), m, onLattice.data(), hostBackLattice.data())) {
        std::printf("a host twin failed: %s\n", sph_last_error());
        return 3;
    }
    auto equal = [](const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(float)); };
    if (!equal(around, hostAround) || !equal(onLattice, hostLattice) || !equal(back, hostBack) || !equal(backFromLattice, hostBackLattice) ||
        std::memcmp(counts.data(), hostCounts.data(), rows * sizeof(uint32_t))) {
        std::printf("a device result differs from its host twin\n");
        return 5;
    }
    // partition of unity against the plain SUM
    SphAggregateConfig plain = fluid.AggregateConfig();
    plain.radius = cfg.radius;
    plain.weight = cfg.weight;
    plain.flags = cfg.flags;
    plain.channels = C;
    std::vector<float> sum, magnitude;
    if (!fluid.Aggregate(info, plain, vel, sum) || !fluid.Aggregate(info, plain, speed, magnitude)) return 3;
    double worst = 0.0;
    for (size_t i = 0; i < rows; ++i)
        for (int c = 0; c < C; ++c) {
            double total = 0.0;
            for (int b = 0; b < B; ++b) total += double(around[(i * B + b) * C + c]);
            const double bound = (double(counts[i]) + 8.0) * std::ldexp(1.0, -23) * double(magnitude[i * C + c]);
            const double err = std::fabs(total - double(sum[i * C + c]));
            if (!(err <= bound)) { std::printf("row %zu channel %d: the planes add up to %.9g, the sum is %.9g\n", i, c, total, double(sum[i * C + c])); return 6; }
            if (bound > 0.0) worst = std::max(worst, err / bound);
        }
    std::printf("particles=%zu lattice=%dx%dx%d planes=%d: four results equal their host twins; partition of unity, largest error / bound %.3g\n", rows, dims[0], dims[1],
                dims[2], B, worst);
    if (argc > 2) {
        std::FILE* f = std::fopen(argv[2], "wb");
        const uint64_t head[4] = {rows, m, uint64_t(C), uint64_t(K)};
        std::vector<SphParams> ps(1, params);
        const bool ok = f && std::fwrite(head, sizeof(head), 1, f) == 1 && put(f, ps) && put(f, now) && put(f, vel) && put(f, points) && put(f, around) &&
                        put(f, onLattice) && put(f, back) && put(f, backFromLattice);
        if (f) std::fclose(f);
        if (!ok) return 7;
    }
    std::printf("continuous_conv OK\n");
    return 0;
}
