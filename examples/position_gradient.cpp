// position_gradient.cpp -- the gradient of a loss in the geometry, through the C++ twin only: the default scene gets a wave impulse and,
// once per frame, the loss L = sum_i rho_i^2 with rho_i = sum_j (R^2 - r_ij^2)^3 (Aggregate of ones: SUM, the poly6 weight, SELF,
// FLUID_ONLY, R = 2 h) is differentiated with respect to every particle's position by AggregatePositionGrad with the upstream
// g_i = dL/drho_i = 2 rho_i.  No edge list, no atomics.  Printed per frame: the largest |dL/dx_k| and the norm of sum_k dL/dx_k.
// Checks, each with an exit code of its own:
//   * every row is finite;
//   * under FLUID_ONLY the row of a ghost particle is +0, bit for bit;
//   * the net gradient vanishes within the rounding bound derived below (translation invariance: L depends on differences of
//     positions only, and every pair term enters twice with opposite signs).
//
// The bound.  With one channel of ones the pair term of row k towards j is e = w1 * g_k * d, w1 = -6 (R^2 - r^2)^2, and row k adds
// e(j -> k) - e(k -> j) for each of its cnt_k neighbours: 2 cnt_k terms, each of magnitude at most |w1| |d_a| g <= 6 R^4 * R * g (g >= 0:
// it is twice a sum of non-negative weights).  On the path of a term the engine rounds the channel dot (one product, one lane add, two
// butterfly adds), d_a, f = w1 * q, f * d_a and the difference of the two directions: fewer than 16 roundings; the row's accumulator
// adds 2 cnt_k more.  The weight's derivative carries an absolute error from the cancellation in t = R^2 - r^2: fl(r^2) is within
// 5 u r^2, so |d(t^2)| <= 2 t (u t + 5 u r^2) + 2 u t^2 <= 10 u t R^2, i.e. at most 10 u of the largest w1.  In all, per component,
//   |sum_k grad_k| <= (2 kmax + 16 + 10 + 4) * u * 6 R^5 * sum_k sum_{j in N(k)} (g_j + g_k) = (2 kmax + 30) * u * 12 R^5 * sum_k cnt_k g_k
// (u = 2^-24; the four spare units cover 1 / (1 - j u) and the float64 sums here; the pair sum is symmetric).  cnt_k comes from
// Aggregate's counts, which include the own slot under SELF: an overestimate.  The norm is at most sqrt(3) times that.
//
//   g++ -std=c++17 -I include examples/position_gradient.cpp -L <pkg dir> -lsph_hip -o position_gradient
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 4;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    SphAggregateConfig cfg = fluid.AggregateConfig();
    cfg.radius = 2.0f * fluid.param_h;
    cfg.weight = SPH_AGGREGATE_WEIGHT_POLY6;
    cfg.flags = SPH_AGGREGATE_SELF | SPH_AGGREGATE_FLUID_ONLY;
    cfg.channels = 1;
    const double R = double(cfg.radius), u = std::ldexp(1.0, -24);
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 4; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        std::vector<SPHParticle> now;
        if (!fluid.Download(now)) return 3;
        const size_t rows = now.size();
        const std::vector<float> ones(rows, 1.0f);
        std::vector<float> rho, g(rows), grad;
        std::vector<uint32_t> counts;
        SphAggregateInfo info;
        if (!fluid.Aggregate(info, cfg, ones, rho, &counts)) { std::printf("Aggregate failed: %s\n", fluid.LastError().c_str()); return 3; }
        for (size_t i = 0; i < rows; ++i) g[i] = 2.0f * rho[i];
        if (!fluid.AggregatePositionGrad(info, cfg, ones, g, grad)) { std::printf("AggregatePositionGrad failed: %s\n", fluid.LastError().c_str()); return 3; }
        if (grad.size() != rows * 3 || info.rows != rows || info.channels != 1 || info.planes != 1) {
            std::printf("the result does not have the shape asked for\n");
            return 4;
        }
        double net[3] = {0.0, 0.0, 0.0}, largest = 0.0, kmax = 0.0, T = 0.0, loss = 0.0;
        size_t ghosts = 0;
        const uint32_t zero[3] = {0u, 0u, 0u};
        for (size_t k = 0; k < rows; ++k) {
            const float* row = &grad[k * 3];
            if (!(std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]))) { std::printf("frame %d: row %zu is not finite\n", frame, k); return 5; }
            if (now[k].isGhost != 0) {
                ghosts += 1;
                if (std::memcmp(row, zero, sizeof(zero)) != 0) { std::printf("frame %d: the row of ghost %zu is not +0\n", frame, k); return 6; }
            }
            for (int a = 0; a < 3; ++a) { net[a] += double(row[a]); largest = std::max(largest, std::fabs(double(row[a]))); }
            kmax = std::max(kmax, double(counts[k]));
            T += double(counts[k]) * double(g[k]);
            loss += double(rho[k]) * double(rho[k]);
        }
        const double norm = std::sqrt(net[0] * net[0] + net[1] * net[1] + net[2] * net[2]);
        const double bound = std::sqrt(3.0) * (2.0 * kmax + 30.0) * u * 12.0 * R * R * R * R * R * T;
        std::printf("frame %d: particles=%zu ghosts=%zu L=%.9g largest |dL/dx|=%.6g |sum dL/dx|=%.3g bound=%.3g kmax=%.0f\n", frame, rows, ghosts, loss, largest, norm, bound,
                    kmax);
        if (!(largest > 0.0)) { std::printf("frame %d: the gradient is all zero\n", frame); return 7; }
        if (!(norm <= bound)) { std::printf("frame %d: the net gradient %.17g exceeds the rounding bound %.17g\n", frame, norm, bound); return 8; }
    }
    std::printf("position_gradient OK\n");
    return 0;
}
