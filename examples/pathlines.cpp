// pathlines.cpp -- passive tracers and their pathlines, through the C++ twin: the 50 000-particle default scene, a horizontal plane
// of 32 x 32 tracers inside the spawned block, ApplyWaveImpulse every frame, 16 fixed-dt substeps per frame as ONE sph_dispatch_n
// call (the tracers are advected inside every substep, on the device).  Per frame: the number of tracers in the fluid
// (fraction >= 0.5) and their mean age.  At the end the pathlines (one snapshot per frame) go into one binary PLY: a vertex
// (x, y, z, age) per snapshot and tracer, an edge between consecutive snapshots of the same tracer.
//
//   g++ -std=c++17 -I include examples/pathlines.cpp -L <pkg dir> -lsph_hip -o pathlines
//   ./pathlines <out.ply> [frames] [particles]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static bool WritePly(const std::string& path, const std::vector<Vec4>& pts, uint32_t snapshots, size_t m) {
    FILE* fh = std::fopen(path.c_str(), "wb");
    if (!fh) return false;
    const size_t edges = snapshots ? size_t(snapshots - 1) * m : 0;
    std::fprintf(fh, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                     "property float age\nelement edge %zu\nproperty int vertex1\nproperty int vertex2\nend_header\n", pts.size(), edges);
    bool ok = pts.empty() || std::fwrite(pts.data(), sizeof(Vec4), pts.size(), fh) == pts.size();
    for (size_t k = 0; ok && k < edges; ++k) {
        const int32_t e[2] = {int32_t(k), int32_t(k + m)};
        ok = std::fwrite(e, sizeof(int32_t), 2, fh) == 2;
    }
    return std::fclose(fh) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: pathlines <out.ply> [frames] [particles]\n"); return 1; }
    const int frames = argc > 2 ? std::atoi(argv[2]) : 4;
    const size_t n = argc > 3 ? (size_t)std::atol(argv[3]) : 50000;
    const int substeps = 16, side = 32;
    SPHFluidGPU fluid(n, /*seed=*/7);
    if (!fluid.LastError().empty()) return 2;
    std::vector<Vec4> seeds;
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i)
            seeds.emplace_back(-5.5f + 9.0f * float(i) / 31.0f, -4.0f, -5.5f + 10.5f * float(j) / 31.0f, 0.0f);
    if (!fluid.SetTracers(seeds, SPH_TRACER_MIDPOINT, uint32_t(frames + 1), uint32_t(substeps))) return 3;
    std::vector<SphTracer> tr;
    float phase = 0.0f;
    for (int frame = 0; frame < frames; ++frame) {
        fluid.ApplyWaveImpulse(1.5f, 3.0f, phase, Vec3(0, 1, 0));
        phase += 4.0f / 60.0f;
        if (sph_dispatch_n(fluid.Handle(), fluid.param_timeStep, substeps) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return 4; }
        if (!fluid.DownloadTracers(tr)) return 5;
        size_t inFluid = 0;
        double age = 0.0;
        for (const SphTracer& t : tr) { inFluid += t.fraction >= 0.5f ? 1 : 0; age += t.age; }
        std::printf("frame %d in_fluid=%zu mean_age=%.6f\n", frame, inFluid, tr.empty() ? 0.0 : age / double(tr.size()));
    }
    std::vector<Vec4> hist;
    uint32_t snapshots = 0;
    uint64_t first = 0;
    if (!fluid.TracerHistory(hist, snapshots, first)) return 6;
    if (snapshots != uint32_t(frames + 1) || first != 0) { std::printf("history: %u snapshots from %llu\n", snapshots, (unsigned long long)first); return 7; }
    if (!WritePly(argv[1], hist, snapshots, fluid.NumTracers())) { std::printf("cannot write %s\n", argv[1]); return 8; }
    std::printf("pathlines OK: %zu tracers, %u snapshots\n", fluid.NumTracers(), snapshots);
    return 0;
}
