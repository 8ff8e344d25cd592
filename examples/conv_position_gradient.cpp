// conv_position_gradient.cpp -- the gradient of a loss over a continuous convolution's basis sums with respect to the positions, through
// the C++ twin only: the default scene gets a wave impulse and runs a few substeps; every particle carries C = 8 features made of its
// velocity; A = AggregateBasis (K = 3, the poly6 weight, FLUID_ONLY, R = 2 h) and the loss L = 1/2 sum A^2, whose upstream is g = A, is
// differentiated with respect to every particle's position by AggregateBasisPositionGrad.  No edge list, no atomics.  Printed: the largest
// |dL/dx_k| and the summed gradient.  Checks, each with an exit code of its own:
//   * every row is finite;
//   * a second call gives the same bytes;
//   * the column sums of the gradient vanish within the rounding bound derived below (translation invariance: L depends on differences
//     of positions only, and every pair term enters twice with opposite signs).
//
// The bound (sph_abi.h "position gradients of the basis sums" for the terms).  Row k adds e(j -> k) - e(k -> j) for each of its cnt_k
// neighbours: 2 cnt_k terms.  A term of target i is e_a = (w1 q) d_a + w p_a with q = sum_c sum_n hat_n g[i][b_n][c] x[j][c] and p_a the
// same with the slopes.  The 8 hats of a candidate are non-negative and sum to 1 and the 8 slopes' magnitudes sum to 2 s, s = half / R,
// so with G_i = max |g[i][.][.]| and X = max |x|: |q| <= C G_i X and |p_a| <= 2 s C G_i X; |w1| <= 6 R^4, |d_a| <= R, |w| <= R^6 and
// 2 s R^6 = (K - 1) R^5, so a term is at most M_i = (5 + K) R^5 C G_i X.  On its path the engine rounds the slope, a corner coefficient's
// two products, g * x, the coefficient's product, the lane's 8 adds (C = 8: one channel per lane) and the butterfly's 3, then d_a, f, f * d_a,
// w * p_a, their sum, the difference of the two directions and the weight's products: 26 roundings, and the row's accumulator 2 cnt_k
// more.  Absolute terms: a hat weight is within eps = (3 (K - 1) + 2) u of the hat function, so a product of three is within
// E3 <= 6.25 eps and of two within E2 <= 4.1 eps, against S = sum_c sum_n |g| |x| <= 8 C G_i X: 6 R^5 E3 S + (K - 1) / 2 R^5 E2 S; and the
// weight's cancellation in t = R^2 - r^2: 60 u R^5 |q| + 15 u R^6 |p_a|.  In units of u R^5 C G_i X that is
//   Y = 48 * 6.25 eps / u + 4 (K - 1) * 4.1 eps / u + 60 + 15 (K - 1).
// Summed over all rows, with sum_k sum_{j in N(k)} (G_k + G_j) = 2 sum_k cnt_k G_k (the relation is symmetric), per component
//   |sum_k grad_k| <= ((2 kmax + 26 + 4) (5 + K) + Y) * u * R^5 * C * X * 2 sum_k cnt_k G_k
// (u = 2^-24; the four spare units cover 1 / (1 - j u) and the float64 sums here).  cnt_k comes from AggregateBasis' counts.
//
//   g++ -std=c++17 -I include examples/conv_position_gradient.cpp -L <pkg dir> -lsph_hip -o conv_position_gradient
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    constexpr int K = 3, C = 8, B = K * K * K;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
    std::vector<SPHParticle> now;
    if (!fluid.Download(now)) return 3;
    const size_t rows = now.size();
    SphBasisConfig cfg = fluid.BasisConfig();
    cfg.radius = 2.0f * fluid.param_h;
    cfg.weight = SPH_AGGREGATE_WEIGHT_POLY6;
    cfg.flags = SPH_AGGREGATE_FLUID_ONLY;
    cfg.channels = C;
    cfg.size = K;
    std::vector<float> x(rows * C);
    double X = 0.0;
    for (size_t k = 0; k < rows; ++k) {
        const float v[3] = {now[k].vel.x, now[k].vel.y, now[k].vel.z};
        const float f[C] = {1.0f, v[0], v[1], v[2], v[0] * v[0], v[1] * v[1], v[2] * v[2], 0.5f};
        for (int c = 0; c < C; ++c) { x[k * C + c] = f[c]; X = std::max(X, std::fabs(double(f[c]))); }
    }
    std::vector<float> A, grad, again;
    std::vector<uint32_t> counts;
    SphAggregateInfo info;
    if (!fluid.AggregateBasis(info, cfg, x, A, &counts)) { std::printf("AggregateBasis failed: %s\n", fluid.LastError().c_str()); return 3; }
    if (!fluid.AggregateBasisPositionGrad(info, cfg, x, A, grad)) { std::printf("AggregateBasisPositionGrad failed: %s\n", fluid.LastError().c_str()); return 3; }
    if (grad.size() != rows * 3 || info.rows != rows || info.channels != C || info.planes != B) {
        std::printf("the result does not have the shape asked for\n");
        return 4;
    }
    if (!fluid.AggregateBasisPositionGrad(info, cfg, x, A, again)) return 3;
    if (again.size() != grad.size() || std::memcmp(again.data(), grad.data(), grad.size() * sizeof(float)) != 0) {
        std::printf("a second call gives other bytes\n");
        return 6;
    }
    double net[3] = {0.0, 0.0, 0.0}, largest = 0.0, kmax = 0.0, T = 0.0, loss = 0.0;
    for (size_t k = 0; k < rows; ++k) {
        const float* row = &grad[k * 3];
        if (!(std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]))) { std::printf("row %zu is not finite\n", k); return 5; }
        for (int a = 0; a < 3; ++a) { net[a] += double(row[a]); largest = std::max(largest, std::fabs(double(row[a]))); }
        double G = 0.0;
        for (int t = 0; t < B * C; ++t) { const double v = double(A[k * B * C + t]); G = std::max(G, std::fabs(v)); loss += 0.5 * v * v; }
        kmax = std::max(kmax, double(counts[k]));
        T += double(counts[k]) * G;
    }
    const double R = double(cfg.radius), u = std::ldexp(1.0, -24), eps = 3.0 * (K - 1) + 2.0;
    const double Y = 48.0 * 6.25 * eps + 4.0 * (K - 1) * 4.1 * eps + 60.0 + 15.0 * (K - 1);
    const double bound = ((2.0 * kmax + 30.0) * (5.0 + K) + Y) * u * R * R * R * R * R * C * X * 2.0 * T;
    std::printf("particles=%zu L=%.9g largest |dL/dx|=%.6g sum dL/dx=(%.3g, %.3g, %.3g) bound=%.3g kmax=%.0f\n", rows, loss, largest, net[0], net[1], net[2], bound, kmax);
    if (!(largest > 0.0)) { std::printf("the gradient is all zero\n"); return 7; }
    for (int a = 0; a < 3; ++a)
        if (!(std::fabs(net[a]) <= bound)) { std::printf("the column sum %.17g exceeds the rounding bound %.17g\n", net[a], bound); return 8; }
    std::printf("conv_position_gradient OK\n");
    return 0;
}
