// surface_mesh.cpp -- the water surface as a closed triangle mesh per frame, through the C++ twin only: the 50 000-particle default
// scene, ApplyWaveImpulse every frame, 16 fixed-dt substeps, then ExtractSurface of `fraction` >= 0.5 on a lattice of spacing h/2
// over the grid box widened by 2h (the default of SPHFluidGPU.surface in engine.py), DownloadSurface, and one binary PLY per frame.
//
//   g++ -std=c++17 -I include examples/surface_mesh.cpp -L <pkg dir> -lsph_hip -o surface_mesh
//   ./surface_mesh <out dir> [frames] [particles]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static bool WritePly(const std::string& path, const std::vector<SphSurfaceVertex>& v, const std::vector<uint32_t>& t3) {
    FILE* fh = std::fopen(path.c_str(), "wb");
    if (!fh) return false;
    std::fprintf(fh, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                     "property float nx\nproperty float ny\nproperty float nz\nelement face %zu\nproperty list uchar uint vertex_indices\nend_header\n",
                 v.size(), t3.size() / 3);
    bool ok = v.empty() || std::fwrite(v.data(), sizeof(SphSurfaceVertex), v.size(), fh) == v.size();
    for (size_t k = 0; ok && k < t3.size(); k += 3) {
        const unsigned char n = 3;
        ok = std::fwrite(&n, 1, 1, fh) == 1 && std::fwrite(&t3[k], sizeof(uint32_t), 3, fh) == 3;
    }
    return std::fclose(fh) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: surface_mesh <out dir> [frames] [particles]\n"); return 1; }
    const std::string dir = argv[1];
    const int frames = argc > 2 ? std::atoi(argv[2]) : 4;
    const size_t n = argc > 3 ? (size_t)std::atol(argv[3]) : 50000;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    const float h = fluid.param_h, s = 0.5f * h;
    const Vec3 origin(fluid.gridMinV.x - 2.0f * h, fluid.gridMinV.y - 2.0f * h, fluid.gridMinV.z - 2.0f * h);
    const int gdims[3] = {fluid.gridSizeX, fluid.gridSizeY, fluid.gridSizeZ};
    int dims[3];
    for (int a = 0; a < 3; ++a) dims[a] = int(std::ceil((fluid.cellSize * float(gdims[a]) + 4.0f * h) / s)) + 1;
    std::vector<SphSurfaceVertex> verts;
    std::vector<uint32_t> tris;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        for (int k = 0; k < 16; ++k) fluid.DispatchCompute(fluid.param_timeStep);
        SphSurface surf;
        if (!fluid.ExtractSurface(origin, Vec3(s, s, s), dims, SPH_FIELD_FRACTION, 0.5f, surf)) {
            std::printf("ExtractSurface failed: %s\n", fluid.LastError().c_str());
            return 3;
        }
        if (!fluid.DownloadSurface(verts, tris)) { std::printf("DownloadSurface failed: %s\n", fluid.LastError().c_str()); return 4; }
        char name[64];
        std::snprintf(name, sizeof(name), "/frame_%04d.ply", frame);
        if (!WritePly(dir + name, verts, tris)) { std::printf("cannot write %s%s\n", dir.c_str(), name); return 5; }
        std::printf("frame %d vertices=%u triangles=%u\n", frame, surf.numVertices, surf.numTriangles);
    }
    std::printf("surface_mesh OK\n");
    return 0;
}
