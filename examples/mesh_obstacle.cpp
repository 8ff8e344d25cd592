// mesh_obstacle.cpp -- a torus given as a triangle mesh, turned into a signed distance lattice on the device and spun in the default box
// tank as a kinematic obstacle, through the C++ twin.  The mesh is built in code (64 x 32 quads, triangles
// counter-clockwise seen from outside); VolumeFromMesh measures it on a lattice of spacing h centred on the body, and a box body of the
// lattice's half extents bound to that volume is the torus.  16 substeps per frame as ONE sph_dispatch_n call.
// Per frame: the mean force the fluid put on the torus (J / t) and the torque about its centre (L / t).
//
// After every frame no fluid particle may lie deeper inside the ANALYTIC torus than the sum of
//   dt |omega| r_max                     the surface moves by at most this in the substep after the projection (section 3e),
//   0.03 h                               the residual of the two-step projection on this lattice (a tube of 7 spacings; the restatement of
//                                        section 3f gives 0.024 h over 120 000 points inside it),
//   3 h^2 / (8 r)                        trilinear interpolation of a distance field of curvature 1 / r, h^2 / (8 r) per axis,
//   (R + r)(1 - cos(pi / 64)) + r (1 - cos(pi / 32))   the mesh is inscribed in the torus: the sagittas of its two families of chords,
//   16 2^-24 (|c| + r_max)               rounding of a projected fp32 position.
// A deeper particle makes the program exit with 9.
//
//   g++ -std=c++17 -I include examples/mesh_obstacle.cpp -L <pkg dir> -lsph_hip -o mesh_obstacle
//   ./mesh_obstacle [substeps] [particles] [omega]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static const double kMajor = 2.2, kMinor = 0.7, kPi = 3.14159265358979323846;
static const int kNu = 64, kNv = 32;

// The torus about the local y axis: vertex (i, j) at angle u = 2 pi i / kNu around the axis and v = 2 pi j / kNv around the tube.
static void TorusMesh(std::vector<float>& verts, std::vector<uint32_t>& tris) {
    for (int i = 0; i < kNu; ++i)
        for (int j = 0; j < kNv; ++j) {
            const double u = 2.0 * kPi * i / kNu, v = 2.0 * kPi * j / kNv, ring = kMajor + kMinor * std::cos(v);
            verts.push_back(float(ring * std::cos(u)));
            verts.push_back(float(kMinor * std::sin(v)));
            verts.push_back(float(ring * std::sin(u)));
        }
    for (int i = 0; i < kNu; ++i)
        for (int j = 0; j < kNv; ++j) {
            const uint32_t a = uint32_t(i * kNv + j), b = uint32_t(((i + 1) % kNu) * kNv + j);
            const uint32_t c = uint32_t(((i + 1) % kNu) * kNv + (j + 1) % kNv), d = uint32_t(i * kNv + (j + 1) % kNv);
            const uint32_t quad[6] = {a, d, c, a, c, b};
            tris.insert(tris.end(), quad, quad + 6);
        }
}

// How deep p lies inside the analytic torus of body b (0 outside), in fp64 on the local frame of b's rotation.
static double TorusDepth(const SphObstacle& b, const SPHParticle& p) {
    const double w = b.rotation[0], x = b.rotation[1], y = b.rotation[2], z = b.rotation[3];
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    const double d[3] = {double(p.pos.x) - b.center[0], double(p.pos.y) - b.center[1], double(p.pos.z) - b.center[2]};
    double l[3];
    for (int j = 0; j < 3; ++j) l[j] = M[j] * d[0] + M[3 + j] * d[1] + M[6 + j] * d[2];
    const double ring = std::sqrt(l[0] * l[0] + l[2] * l[2]) - kMajor;
    const double depth = kMinor - std::sqrt(ring * ring + l[1] * l[1]);
    return depth > 0.0 ? depth : 0.0;
}

int main(int argc, char** argv) {
    const int total = argc > 1 ? std::atoi(argv[1]) : 160;
    const size_t n = argc > 2 ? (size_t)std::atol(argv[2]) : 50000;
    const float omega = argc > 3 ? (float)std::atof(argv[3]) : 3.0f;
    const int substeps = 16;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    for (int i = 0; i < 30; ++i) fluid.DispatchCompute();                  // let the spawned block settle a little first

    std::vector<float> verts;
    std::vector<uint32_t> tris;
    TorusMesh(verts, tris);
    const float h = 0.1f;
    const int dims[3] = {63, 19, 63};                                      // the torus's box (5.8 x 1.4 x 5.8) and two spacings of margin
    const Vec3 center(fluid.param_boxCenter.x, fluid.param_boxCenter.y - fluid.param_boxHalf.y + 3.0f, fluid.param_boxCenter.z);
    int volume = -1;
    Vec3 half;
    if (!fluid.VolumeFromMesh(verts, tris, Vec3(0.0f, 0.0f, 0.0f), h, dims, volume, half)) { std::printf("%s\n", fluid.LastError().c_str()); return 3; }
    SphObstacle body;
    sph_obstacle_default(&body);
    body.shape = SPH_OBSTACLE_BOX;
    body.size[0] = half.x; body.size[1] = half.y; body.size[2] = half.z;
    body.center[0] = center.x; body.center[1] = center.y; body.center[2] = center.z;
    body.omega[0] = omega;                                                 // the ring tumbles about x through the fluid
    if (!fluid.SetObstacles({body}) || !fluid.BindObstacleVolume(0, volume)) { std::printf("%s\n", fluid.LastError().c_str()); return 3; }

    const float dt = fluid.param_timeStep;
    const double rmax = kMajor + kMinor;
    const double shape = 0.03 * h + 3.0 * double(h) * h / (8.0 * kMinor) + rmax * (1.0 - std::cos(kPi / kNu)) + kMinor * (1.0 - std::cos(kPi / kNv));
    std::vector<SPHParticle> recs;
    std::vector<SphObstacle> cur;
    std::vector<double> J;
    for (int done = 0, frame = 0; done < total; ++frame) {
        const int now = std::min(substeps, total - done);
        if (sph_dispatch_n(fluid.Handle(), dt, now) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        done += now;
        double t = 0.0;
        uint64_t steps = 0;
        if (!fluid.ObstacleImpulses(J, t, steps, /*reset=*/true) || !fluid.GetObstacles(cur) || cur.size() != 1 || !(t > 0.0)) return 5;
        if (!fluid.Download(recs)) return 6;
        const double scale = std::fabs(cur[0].center[0]) + std::fabs(cur[0].center[1]) + std::fabs(cur[0].center[2]) + rmax;
        const double tol = double(dt) * std::fabs(double(omega)) * rmax + shape + 16.0 * std::ldexp(1.0, -24) * scale;
        double deepest = 0.0;
        for (const SPHParticle& p : recs)
            if (p.isGhost == 0) deepest = std::fmax(deepest, TorusDepth(cur[0], p));
        std::printf("frame %d substeps=%llu force=(%.6f, %.6f, %.6f) torque=(%.6f, %.6f, %.6f) deepest=%.3g allowed=%.3g\n", frame,
                    (unsigned long long)steps, J[0] / t, J[1] / t, J[2] / t, J[3] / t, J[4] / t, J[5] / t, deepest, tol);
        if (deepest > tol) { std::printf("a fluid particle lies %.6g inside the torus\n", deepest); return 9; }
    }
    std::printf("mesh_obstacle OK\n");
    return 0;
}
