// stirred_tank.cpp -- a box paddle spinning about y in the default box tank, through the C++ twin.  16 substeps
// per frame as ONE sph_dispatch_n call: the engine keeps the fluid out of the paddle and turns it on the device, with no host round trip.
// Per frame: the mean force the fluid put on the paddle (J / t) and the torque about y (L_y / t, about the paddle's centre).
//
// After every frame no fluid particle may lie inside the paddle deeper than the paddle's surface moves in one substep plus the rounding
// of a projected fp32 position: the obstacle step leaves every particle outside the pose it used, and the pose then advances by one
// substep (dt |omega| r_max, r_max the half diagonal).  A deeper particle makes the program exit with 9.
//
//   g++ -std=c++17 -I include examples/stirred_tank.cpp -L <pkg dir> -lsph_hip -o stirred_tank
//   ./stirred_tank [frames] [particles] [omega]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

// How deep p lies inside box paddle b (0 outside), in fp64 on the local frame of b's rotation.
static double BoxDepth(const SphObstacle& b, const SPHParticle& p) {
    const double w = b.rotation[0], x = b.rotation[1], y = b.rotation[2], z = b.rotation[3];
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    const double d[3] = {double(p.pos.x) - b.center[0], double(p.pos.y) - b.center[1], double(p.pos.z) - b.center[2]};
    double depth = 1e300;
    for (int j = 0; j < 3; ++j) {
        const double l = M[j] * d[0] + M[3 + j] * d[1] + M[6 + j] * d[2];
        depth = std::fmin(depth, double(b.size[j]) - std::fabs(l));
    }
    return depth > 0.0 ? depth : 0.0;
}

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
    const float dt = fluid.param_timeStep;
    const double rmax = std::sqrt(double(paddle.size[0]) * paddle.size[0] + double(paddle.size[1]) * paddle.size[1] + double(paddle.size[2]) * paddle.size[2]);
    std::vector<SPHParticle> recs;
    std::vector<SphObstacle> cur;
    std::vector<double> J;
    for (int frame = 0; frame < frames; ++frame) {
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        double t = 0.0;
        uint64_t steps = 0;
        if (!fluid.ObstacleImpulses(J, t, steps, /*reset=*/true) || !fluid.GetObstacles(cur) || cur.size() != 1 || !(t > 0.0)) return 5;
        if (!fluid.Download(recs)) return 6;
        const double scale = std::fabs(cur[0].center[0]) + std::fabs(cur[0].center[1]) + std::fabs(cur[0].center[2]) + rmax;
        const double tol = double(dt) * std::fabs(double(omega)) * rmax + 16.0 * std::ldexp(1.0, -24) * scale;
        double deepest = 0.0;
        for (const SPHParticle& p : recs)
            if (p.isGhost == 0) deepest = std::fmax(deepest, BoxDepth(cur[0], p));
        std::printf("frame %d substeps=%llu force=(%.6f, %.6f, %.6f) torque_y=%.6f deepest=%.3g allowed=%.3g\n", frame, (unsigned long long)steps,
                    J[0] / t, J[1] / t, J[2] / t, J[4] / t, deepest, tol);
        if (deepest > tol) { std::printf("a fluid particle lies %.6g inside the paddle\n", deepest); return 9; }
    }
    std::printf("stirred_tank OK\n");
    return 0;
}
