// range_scan.cpp -- a range sensor above the tank, through the C++ twin only: the default scene gets a wave impulse, then once per
// frame a 64 x 64 sheet of parallel rays is cast straight down from above the grid's box against the particles (spheres of radius
// h / 4).  Prints hits, misses and the lowest, mean and highest hit height, and checks the hits: an id is a particle id, a miss is
// (-1, +inf, zeros), a hit's t lies in [tmin, tmax], the counts are RaysInfo's, and the hit point lies on the sphere of its particle
// within the bound derived below.  Exits non-zero if one of them fails.  No image is written: the result is numbers.
//
//   g++ -std=c++17 -I include examples/range_scan.cpp -L <pkg dir> -lsph_hip -o range_scan
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

// How far | |pos - x|^2 - r^2 | may be from 0, from the arithmetic of a cast, e = 2^-24 the unit roundoff of fp32.
// With L = x - o, D = |d|, q' = L - tca d for the COMPUTED tca: |x - (o + t d)|^2 = |q'|^2 + ((t - tca) D)^2 - 2 (t - tca) q'.d exactly, and
// the cast sets ((t - tca) D)^2 = thc^2 a = r2 - d2 up to three roundings (3 e r^2, plus e r^2 for r2 = r * r).  What is left:
//   the cross term    q'.d = a (tca_true - tca); tca is a dot3 of rounded L (e |L| per axis) times 1 / a: |tca_true - tca| D <= 6 e |L|,
//                     and |t - tca| D <= r: 2 r * 6 e |L| = 12 e r |L|
//   d2 against |q'|^2 L's rounding moves q' by e |L| (2 sqrt(3) e r |L|), the three fmaf by e r, the dot3 by 3 e r^2: < 4 e r |L| + 5 e r^2
//   t = tca - thc     one rounding, e |t|, moves the point by e T, T = |t| D: 2 r e T
//   pos = fmaf(t,d,o) one rounding per axis, e M with M the largest |pos| component: 2 sqrt(3) r e M < 4 e r M
// Sum: e r (16 |L| + 2 T + 4 M) + 9 e r^2.  Second-order terms are a factor e smaller and lie inside the rounding-up of the constants
// above (2 sqrt(3) -> 4, 5 e |L| -> 6 e |L|).
static double hit_bound(double r, double absL, double T, double M) {
    const double e = std::ldexp(1.0, -24);
    return e * r * (16.0 * absL + 2.0 * T + 4.0 * M) + 9.0 * e * r * r;
}

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : 50000;
    const int frames = argc > 2 ? std::atoi(argv[2]) : 6;
    const int side = 64;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    fluid.ApplyWaveImpulse(1.5f, 3.0f, 0.25f, Vec3(0.0f, 1.0f, 0.0f));
    fluid.ComputeGridExtents();
    const float r = 0.25f * fluid.param_h;
    const float x0 = fluid.gridMinV.x, z0 = fluid.gridMinV.z, top = fluid.gridMinV.y + fluid.cellSize * float(fluid.gridSizeY) + 1.0f;
    const float ex = fluid.cellSize * float(fluid.gridSizeX), ez = fluid.cellSize * float(fluid.gridSizeZ);
    const float tmin = 0.0f, tmax = fluid.cellSize * float(fluid.gridSizeY) + 2.0f;
    std::vector<float> rays;
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const float ray[8] = {x0 + ex * (float(i) + 0.5f) / float(side), top, z0 + ez * (float(j) + 0.5f) / float(side), tmin, 0.0f, -1.0f, 0.0f, tmax};
            rays.insert(rays.end(), ray, ray + 8);
        }
    std::vector<SphRayHit> hits;
    std::vector<SPHParticle> now;
    for (int frame = 0; frame < frames; ++frame) {
        for (int s = 0; s < 8; ++s) fluid.DispatchCompute(fluid.param_timeStep);
        SphRaysInfo info;
        if (!fluid.CastRays(rays, info, r) || !fluid.DownloadRayHits(hits) || !fluid.Download(now)) {
            std::printf("CastRays failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        if (info.rays != uint64_t(side * side) || hits.size() != size_t(side * side) || info.voidRays != 0) {
            std::printf("the info does not describe the hits\n");
            return 4;
        }
        uint64_t nHit = 0;
        double lo = 0.0, hi = 0.0, sum = 0.0, worst = 0.0;
        for (size_t i = 0; i < hits.size(); ++i) {
            const SphRayHit& h = hits[i];
            if (h.id == -1) {
                const bool zeros = h.pos[0] == 0.0f && h.pos[1] == 0.0f && h.pos[2] == 0.0f && h.normal[0] == 0.0f && h.normal[1] == 0.0f && h.normal[2] == 0.0f;
                if (!(std::isinf(h.t) && h.t > 0.0f) || !zeros) { std::printf("ray %zu: a miss is not (-1, +inf, zeros)\n", i); return 5; }
                continue;
            }
            if (h.id < 0 || size_t(h.id) >= now.size()) { std::printf("ray %zu: id %d is out of range\n", i, h.id); return 9; }
            if (!(h.t >= tmin && h.t <= tmax)) { std::printf("ray %zu: t = %g outside [%g, %g]\n", i, double(h.t), double(tmin), double(tmax)); return 6; }
            const SPHParticle& p = now[size_t(h.id)];
            const double c[3] = {p.pos.x, p.pos.y, p.pos.z}, o[3] = {rays[8 * i], rays[8 * i + 1], rays[8 * i + 2]};
            double dist2 = 0.0, absL = 0.0, M = 0.0;
            for (int a = 0; a < 3; ++a) {
                dist2 += (double(h.pos[a]) - c[a]) * (double(h.pos[a]) - c[a]);
                absL += (c[a] - o[a]) * (c[a] - o[a]);
                M = std::max(M, std::fabs(double(h.pos[a])));
            }
            absL = std::sqrt(absL);
            const double err = std::fabs(dist2 - double(r) * double(r)), bound = hit_bound(double(r), absL, std::fabs(double(h.t)), M);   // (|d| = 1)
            if (!(err <= bound)) { std::printf("ray %zu: | |pos - x|^2 - r^2 | = %g above the bound %g\n", i, err, bound); return 8; }
            worst = std::max(worst, err / bound);
            const double y = double(h.pos[1]);
            lo = nHit ? std::min(lo, y) : y;
            hi = nHit ? std::max(hi, y) : y;
            sum += y;
            nHit += 1;
        }
        if (nHit != info.hits) { std::printf("hits = %llu, the rows hold %llu\n", (unsigned long long)info.hits, (unsigned long long)nHit); return 7; }
        std::printf("frame %d rays=%d hits=%llu misses=%llu height min=%.5f mean=%.5f max=%.5f (sphere error / bound <= %.3f)\n", frame, side * side,
                    (unsigned long long)nHit, (unsigned long long)(hits.size() - nHit), lo, nHit ? sum / double(nHit) : 0.0, hi, worst);
    }
    std::printf("range_scan OK\n");
    return 0;
}
