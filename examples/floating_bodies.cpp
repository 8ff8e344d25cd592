// floating_bodies.cpp -- a light box, a heavier sphere and a sinking capsule dropped into the default scene, through the C++ twin
// (DESIGN.md section 3g).  The bodies are dynamic: the engine turns the fluid's impulses, gravity and the container into their motion on
// the device, so 16 substeps per frame run as ONE sph_dispatch_n call with no host round trip.
// Per frame: the height of every body and the fluid's share of its weight (mean J_y per substep over M g dt).
//
// The program exits non-zero on a record that is not finite, on a body whose support points lie outside the container box by more than
// the body moves in one substep, and on a fluid particle deeper inside a body than the body's surface moves in one substep plus the
// contact shift of that substep (both bounded by dt (|V| + |omega| r_max), taken at the speeds the frame's last substep left) plus the
// rounding of a projected fp32 position.
//
//   g++ -std=c++17 -I include examples/floating_bodies.cpp -L <pkg dir> -lsph_hip -o floating_bodies
//   ./floating_bodies [frames] [particles]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static void Matrix(const SphObstacle& b, double M[9]) {
    const double w = b.rotation[0], x = b.rotation[1], y = b.rotation[2], z = b.rotation[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) M[i] = R[i];
}

// How deep p lies inside body b (0 outside), in fp64 on the local frame of b's rotation.
static double Depth(const SphObstacle& b, const SPHParticle& p) {
    double M[9], l[3];
    Matrix(b, M);
    const double d[3] = {double(p.pos.x) - b.center[0], double(p.pos.y) - b.center[1], double(p.pos.z) - b.center[2]};
    for (int j = 0; j < 3; ++j) l[j] = M[j] * d[0] + M[3 + j] * d[1] + M[6 + j] * d[2];
    double depth;
    if (b.shape == SPH_OBSTACLE_SPHERE) depth = b.size[0] - std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    else if (b.shape == SPH_OBSTACLE_BOX) depth = std::fmin(std::fmin(b.size[0] - std::fabs(l[0]), b.size[1] - std::fabs(l[1])), b.size[2] - std::fabs(l[2]));
    else {
        const double s = std::fmin(std::fmax(l[1], -double(b.size[1])), double(b.size[1]));
        depth = b.size[0] - std::sqrt(l[0] * l[0] + (l[1] - s) * (l[1] - s) + l[2] * l[2]);
    }
    return depth > 0.0 ? depth : 0.0;
}

static double RMax(const SphObstacle& b) {
    if (b.shape == SPH_OBSTACLE_SPHERE) return b.size[0];
    if (b.shape == SPH_OBSTACLE_BOX) return std::sqrt(double(b.size[0]) * b.size[0] + double(b.size[1]) * b.size[1] + double(b.size[2]) * b.size[2]);
    return double(b.size[0]) + b.size[1];
}

// How far the body reaches beyond the container box (axis aligned in the default scene), 0 inside.
static double Outside(const SphObstacle& b, const Vec3& c, const Vec3& h) {
    double M[9];
    Matrix(b, M);
    const double bc[3] = {c.x, c.y, c.z}, bh[3] = {h.x, h.y, h.z};
    double worst = 0.0;
    const int np = b.shape == SPH_OBSTACLE_SPHERE ? 1 : (b.shape == SPH_OBSTACLE_CAPSULE ? 2 : 8);
    const double rad = b.shape == SPH_OBSTACLE_BOX ? 0.0 : b.size[0];
    for (int i = 0; i < np; ++i) {
        double l[3] = {0.0, 0.0, 0.0};
        if (b.shape == SPH_OBSTACLE_CAPSULE) l[1] = i ? b.size[1] : -b.size[1];
        if (b.shape == SPH_OBSTACLE_BOX) { l[0] = (i & 1) ? b.size[0] : -b.size[0]; l[1] = (i & 2) ? b.size[1] : -b.size[1]; l[2] = (i & 4) ? b.size[2] : -b.size[2]; }
        for (int a = 0; a < 3; ++a) {
            const double p = b.center[a] + M[3 * a] * l[0] + M[3 * a + 1] * l[1] + M[3 * a + 2] * l[2];
            worst = std::fmax(worst, std::fabs(p - bc[a]) + rad - bh[a]);
        }
    }
    return worst;
}

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 20;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const int substeps = 16;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    for (int i = 0; i < 200; ++i) fluid.DispatchCompute();                 // let the spawned block fall into a pool first
    const float rho = fluid.param_restDensity;
    const float top = fluid.param_boxCenter.y - fluid.param_boxHalf.y + 2.5f;
    std::vector<SphObstacle> bodies(3);
    std::vector<SphObstacleDynamics> dyn(3);
    for (int i = 0; i < 3; ++i) {
        sph_obstacle_default(&bodies[i]);
        sph_obstacle_dynamics_default(&dyn[i]);
        bodies[i].center[0] = fluid.param_boxCenter.x + 4.0f * float(i - 1);
        bodies[i].center[1] = top;
        bodies[i].center[2] = fluid.param_boxCenter.z;
    }
    // a light box, tilted: m = 8 a b c rho, I_xx = m (b^2 + c^2) / 3
    bodies[0].shape = SPH_OBSTACLE_BOX;
    bodies[0].size[0] = 0.8f; bodies[0].size[1] = 0.3f; bodies[0].size[2] = 0.5f;
    bodies[0].rotation[0] = 0.95f; bodies[0].rotation[3] = 0.3f;
    {
        const float a = 0.8f, b = 0.3f, c = 0.5f, m = 0.3f * rho * 8.0f * a * b * c;
        dyn[0].mass = m;
        dyn[0].inertia[0] = m * (b * b + c * c) / 3.0f; dyn[0].inertia[1] = m * (a * a + c * c) / 3.0f; dyn[0].inertia[2] = m * (a * a + b * b) / 3.0f;
    }
    // a heavier sphere that still floats: m = 4/3 pi R^3 rho, I = 2/5 m R^2
    bodies[1].shape = SPH_OBSTACLE_SPHERE;
    bodies[1].size[0] = 0.5f;
    {
        const float R = 0.5f, m = 0.6f * rho * 4.18879020f * R * R * R;
        dyn[1].mass = m;
        dyn[1].inertia[0] = dyn[1].inertia[1] = dyn[1].inertia[2] = 0.4f * m * R * R;
    }
    // a capsule three times as dense as the fluid: a cylinder and two half spheres
    bodies[2].shape = SPH_OBSTACLE_CAPSULE;
    bodies[2].size[0] = 0.3f; bodies[2].size[1] = 0.4f;
    bodies[2].rotation[0] = 0.9f; bodies[2].rotation[1] = 0.4f;
    {
        const float r = 0.3f, L = 0.4f, d = 3.0f * rho, pi = 3.14159265f;
        const float mc = d * pi * r * r * 2.0f * L, mh = d * (2.0f / 3.0f) * pi * r * r * r;
        dyn[2].mass = mc + 2.0f * mh;
        dyn[2].inertia[1] = 0.5f * mc * r * r + 2.0f * (0.4f * mh * r * r);
        dyn[2].inertia[0] = dyn[2].inertia[2] =
            mc * (3.0f * r * r + 4.0f * L * L) / 12.0f + 2.0f * (mh * (0.4f - 9.0f / 64.0f) * r * r + mh * (L + 0.375f * r) * (L + 0.375f * r));
    }
    if (!fluid.SetObstacles(bodies)) return 3;
    for (int i = 0; i < 3; ++i)
        if (!fluid.SetObstacleDynamics(i, &dyn[i])) { std::printf("%s\n", fluid.LastError().c_str()); return 3; }
    const float dt = fluid.param_timeStep;
    const double g = std::fabs(double(fluid.param_gravityY));
    std::vector<SPHParticle> recs;
    std::vector<SphObstacle> cur;
    std::vector<double> J;
    for (int frame = 0; frame < frames; ++frame) {
        if (sph_dispatch_n(fluid.Handle(), dt, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        double t = 0.0;
        uint64_t steps = 0;
        if (!fluid.ObstacleImpulses(J, t, steps, /*reset=*/true) || !fluid.GetObstacles(cur) || cur.size() != 3 || !(t > 0.0)) return 5;
        if (!fluid.Download(recs)) return 6;
        std::printf("frame %d substeps=%llu", frame, (unsigned long long)steps);
        for (int i = 0; i < 3; ++i) {
            const SphObstacle& b = cur[i];
            double speed = 0.0, spin = 0.0, scale = RMax(b);
            bool finite = true;
            for (int a = 0; a < 3; ++a) {
                finite = finite && std::isfinite(b.center[a]) && std::isfinite(b.vel[a]) && std::isfinite(b.omega[a]);
                speed += double(b.vel[a]) * b.vel[a]; spin += double(b.omega[a]) * b.omega[a]; scale += std::fabs(b.center[a]);
            }
            for (int a = 0; a < 4; ++a) finite = finite && std::isfinite(b.rotation[a]);
            for (int a = 0; a < 6; ++a) finite = finite && std::isfinite(J[6 * i + a]);
            if (!finite) { std::printf("\nbody %d: a record is not finite\n", i); return 7; }
            const double move = 2.0 * double(dt) * (std::sqrt(speed) + std::sqrt(spin) * RMax(b)) + 16.0 * std::ldexp(1.0, -24) * scale;
            const double out = Outside(b, fluid.param_boxCenter, fluid.param_boxHalf);
            double deepest = 0.0;
            for (const SPHParticle& p : recs)
                if (p.isGhost == 0) deepest = std::fmax(deepest, Depth(b, p));
            std::printf(" | body %d y=%.4f share=%.3f deepest=%.3g", i, b.center[1], (J[6 * i + 1] / double(steps)) / (double(dyn[i].mass) * g * dt), deepest);
            if (out > move) { std::printf("\nbody %d reaches %.6g outside the container (allowed %.3g)\n", i, out, move); return 8; }
            if (deepest > move) { std::printf("\na fluid particle lies %.6g inside body %d (allowed %.3g)\n", deepest, i, move); return 9; }
        }
        std::printf("\n");
    }
    std::printf("floating_bodies OK\n");
    return 0;
}
