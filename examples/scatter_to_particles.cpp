// scatter_to_particles.cpp -- the point -> particle transfer, through the C++ twin only: the default scene gets a wave impulse, the
// velocity is gathered onto a coarse lattice (QueryAggregate, SUM with the poly6 weight) and what the lattice holds is handed back to the
// particles by the exact transpose of that gather (QueryAggregateAdjoint): every particle sums, in a fixed order and without atomics,
// what the lattice points within R of it carry.  Checks, each with an exit code of its own:
//   * the dot-product identity <A x, g> = <x, A^T g> for g = A x, within the bound derived below;
//   * under FLUID_ONLY the row of a ghost particle, and the row of a particle with a non-finite position, is all zero;
//   * for particle targets the adjoint of a plain SUM is Aggregate of the same tensor, byte for byte.
//
// The bound.  y = fl(A x) and z = fl(A^T g) are fp32 recursive sums of at most kmax terms, each term one more rounded product:
// |y - A x| <= gamma_(kmax + 1) A|x| and |z - A^T g| <= gamma_(kmax + 1) A^T|g| componentwise (gamma_j = j u / (1 - j u), u = 2^-24;
// the weights are >= 0 and enter both sides as the same fp32 numbers).  Because <A x, g> = <x, A^T g> exactly,
//   |<y, g> - <x, z>| <= |<y - A x, g>| + |<x, A^T g - z>| <= 2 gamma_(kmax + 1) T,   T = <A|x|, |g|> = <|x|, A^T|g|>,
// and 2 gamma_(kmax + 1) <= (kmax + 8) 2^-23.  T itself comes from the engine (the gather of |x|, in fp32: short of the exact T by at
// most the factor 1 - gamma_(kmax + 1), which the seven spare units of kmax + 8 cover for every kmax below 2^20); kmax is the largest
// count on either side: the most particles around a lattice point and the most lattice points around a particle.
//
//   g++ -std=c++17 -I include examples/scatter_to_particles.cpp -L <pkg dir> -lsph_hip -o scatter_to_particles
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int C = 3;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
    std::vector<SPHParticle> now;
    if (!fluid.Download(now)) return 3;
    const size_t rows = now.size();
    std::vector<float> vel(rows * C), speed(rows * C);
    for (size_t i = 0; i < rows; ++i) {
        vel[i * C] = now[i].vel.x; vel[i * C + 1] = now[i].vel.y; vel[i * C + 2] = now[i].vel.z;
        for (int c = 0; c < C; ++c) speed[i * C + c] = std::fabs(vel[i * C + c]);
    }
    // a coarse lattice over the grid's box, spacing 1.5 h, gathered within R = 2 h
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
    SphAggregateConfig cfg = fluid.AggregateConfig();
    cfg.radius = 2.0f * fluid.param_h;
    cfg.weight = SPH_AGGREGATE_WEIGHT_POLY6;
    cfg.flags = SPH_AGGREGATE_FLUID_ONLY;
    cfg.channels = C;
    SphAggregateInfo info;
    std::vector<float> onLattice, magnitude, back, degree;
    std::vector<uint32_t> counts;
    if (!fluid.Aggregate(info, cfg, vel, onLattice, &counts, points.data(), m) || !fluid.Aggregate(info, cfg, speed, magnitude, nullptr, points.data(), m) ||
        !fluid.AggregateAdjoint(info, cfg, onLattice, back, points.data(), m)) {
        std::printf("the transfer failed: %s\n", fluid.LastError().c_str());
        return 3;
    }
    if (onLattice.size() != m * C || back.size() != rows * C || info.rows != rows || info.channels != C) {
        std::printf("the results do not have the shapes asked for\n");
        return 4;
    }
    // the most lattice points around one particle: the adjoint of ones with the weight ONE counts them exactly
    SphAggregateConfig count = cfg;
    count.weight = SPH_AGGREGATE_WEIGHT_ONE;
    count.channels = 1;
    if (!fluid.AggregateAdjoint(info, count, std::vector<float>(m, 1.0f), degree, points.data(), m)) return 3;
    double kmax = 0.0, lhs = 0.0, rhs = 0.0, T = 0.0;
    for (size_t p = 0; p < m; ++p) kmax = std::max(kmax, double(counts[p]));
    for (size_t i = 0; i < rows; ++i) kmax = std::max(kmax, double(degree[i]));
    for (size_t t = 0; t < m * C; ++t) { lhs += double(onLattice[t]) * double(onLattice[t]); T += double(magnitude[t]) * std::fabs(double(onLattice[t])); }
    for (size_t t = 0; t < rows * C; ++t) rhs += double(vel[t]) * double(back[t]);
    const double bound = (kmax + 8.0) * std::ldexp(1.0, -23) * T;
    std::printf("particles=%zu lattice=%dx%dx%d kmax=%.0f <Ax, g>=%.9g <x, A^T g>=%.9g |difference|/bound=%.3g\n", rows, dims[0], dims[1], dims[2], kmax, lhs, rhs,
                bound > 0.0 ? std::fabs(lhs - rhs) / bound : 0.0);
    if (!(T > 0.0) || !(std::fabs(lhs - rhs) <= bound)) {
        std::printf("the dot-product identity fails: |%.17g - %.17g| > %.17g\n", lhs, rhs, bound);
        return 5;
    }
    size_t quiet = 0;
    for (size_t i = 0; i < rows; ++i) {
        const bool finite = std::isfinite(now[i].pos.x) && std::isfinite(now[i].pos.y) && std::isfinite(now[i].pos.z);
        if (now[i].isGhost == 0 && finite) continue;
        quiet += 1;
        for (int c = 0; c < C; ++c)
            if (back[i * C + c] != 0.0f || degree[i] != 0.0f) { std::printf("particle %zu: a ghost or non-finite row is not zero\n", i); return 6; }
    }
    // particle targets: the relation and the weights are symmetric, so the adjoint of a plain SUM is the forward
    std::vector<float> forward, adjoint;
    if (!fluid.Aggregate(info, cfg, vel, forward) || !fluid.AggregateAdjoint(info, cfg, vel, adjoint)) return 3;
    if (forward.size() != adjoint.size() || std::memcmp(forward.data(), adjoint.data(), forward.size() * sizeof(float)) != 0) {
        std::printf("the particle-target adjoint of a plain SUM differs from Aggregate of the same tensor\n");
        return 7;
    }
    std::printf("ghost or non-finite rows=%zu, all zero; adjoint == forward on %zu floats\n", quiet, forward.size());
    std::printf("scatter_to_particles OK\n");
    return 0;
}
