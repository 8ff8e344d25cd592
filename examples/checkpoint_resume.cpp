// checkpoint_resume.cpp -- checkpoints through the C++ twin: the stirred tank (a box paddle spinning in the
// default scene, stirred_tank.cpp) with a gate across its middle, a probe monitor and tracers.  The same run twice:
//   * a + b substeps without a break;
//   * a substeps, SaveState to a file, the engine destroyed, a new engine of another size, LoadState from the file, b more substeps.
// It prints the section digests of both ends.
//
// The program exits non-zero if
//   * a digest of the resumed run differs from the uninterrupted run's (exit 6);
//   * PeekState's checksums of the file differ from StateDigest taken at the save (exit 7);
//   * a blob with one flipped byte is accepted by PeekState or LoadState (exit 8);
//   * the records, the tracers, the gate books or the paddle's pose of the two ends differ in a byte (exit 9).
//
//   g++ -std=c++17 -I include examples/checkpoint_resume.cpp -L <pkg dir> -lsph_hip -o checkpoint_resume
//   ./checkpoint_resume [a] [b] [particles] [file]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "SPHFluidGPU_hip.hpp"

using namespace MATH;

static const char* kNames[SPH_STATE_SECTION_COUNT] = {"core", "particles", "tracers", "diffuse", "scalars", "obstacles", "gates", "monitors"};

static bool set_up(SPHFluidGPU& fluid) {
    const Vec3 c = fluid.param_boxCenter, half = fluid.param_boxHalf;
    SphObstacle paddle;
    sph_obstacle_default(&paddle);
    paddle.shape = SPH_OBSTACLE_BOX;
    paddle.size[0] = 3.0f; paddle.size[1] = 2.5f; paddle.size[2] = 0.4f;   // a blade 6 wide, 5 high, 0.8 thick
    paddle.center[0] = c.x; paddle.center[1] = c.y - half.y + 3.0f; paddle.center[2] = c.z;
    paddle.omega[1] = 4.0f;
    if (!fluid.SetObstacles({paddle})) return false;
    SphGate gate;
    std::memset(&gate, 0, sizeof(gate));
    gate.shape = SPH_GATE_RECT;
    gate.center[0] = c.x; gate.center[1] = c.y - half.y + 2.0f; gate.center[2] = c.z;
    gate.u[1] = 2.0f; gate.v[2] = half.z;                                  // the plane x = centre, two units up from the floor
    std::vector<Vec4> probes, tracers;
    for (int i = 0; i < 8; ++i) probes.push_back(Vec4(c.x + 0.5f * half.x * float(i - 4) / 4.0f, c.y - half.y + 1.0f, c.z, 0.0f));
    for (int i = 0; i < 200; ++i)
        tracers.push_back(Vec4(c.x + 0.6f * half.x * float(i % 20 - 10) / 10.0f, c.y - half.y + 0.5f + 0.1f * float(i / 20), c.z + 0.3f * half.z * float(i % 7 - 3) / 3.0f, 0.0f));
    SphMonitorConfig cfg = SPHFluidGPU::MonitorConfig();
    cfg.every = 4; cfg.history = 8; cfg.stride = 1; cfg.ringPoints = 8;
    return fluid.SetGates({gate}, 16, 2) && fluid.SetMonitor(0, probes, cfg) && fluid.SetTracers(tracers, SPH_TRACER_MIDPOINT, 4, 3);
}

// `steps` substeps from substep number `from`, in chunks that end at the multiples of eight: one dispatch, the rest in a sph_dispatch_n call.
static bool run(SPHFluidGPU& fluid, int from, int steps) {
    for (int s = from; s < from + steps;) {
        int chunk = 8 - s % 8;
        if (chunk > from + steps - s) chunk = from + steps - s;
        fluid.DispatchCompute();                                            // (the members are pushed once per chunk)
        if (chunk > 1 && sph_dispatch_n(fluid.Handle(), -1.0f, chunk - 1) != SPH_OK) { std::printf("sph_dispatch_n failed: %s\n", sph_last_error()); return false; }
        s += chunk;
    }
    return fluid.LastError().empty();
}

struct End {
    SphStateDigest digest;
    std::vector<SPHParticle> records;
    std::vector<SphTracer> tracers;
    std::vector<SphGateBooks> books;
    std::vector<SphObstacle> bodies;
    double time = 0.0;
    uint64_t substeps = 0;
};
static bool end_of(SPHFluidGPU& fluid, End& e) {
    return fluid.StateDigest(e.digest) && fluid.Download(e.records) && fluid.DownloadTracers(e.tracers) && fluid.GateBooks(e.books, e.time, e.substeps) &&
           fluid.GetObstacles(e.bodies);
}
static void print_digest(const char* what, const SphStateDigest& d) {
    std::printf("%s\n", what);
    for (int i = 0; i < SPH_STATE_SECTION_COUNT; ++i)
        if (d.sections & (1u << i)) std::printf("  %-10s %016llx %016llx\n", kNames[i], (unsigned long long)d.sum[i][0], (unsigned long long)d.sum[i][1]);
}

int main(int argc, char** argv) {
    const int a = argc > 1 ? std::atoi(argv[1]) : 21;
    const int b = argc > 2 ? std::atoi(argv[2]) : 19;
    const size_t n = argc > 3 ? (size_t)std::atol(argv[3]) : 20000;
    const std::string path = argc > 4 ? argv[4] : "checkpoint_resume.sphstate";

    End whole;
    {
        SPHFluidGPU fluid(n, /*seed=*/7);
        if (!fluid.LastError().empty() || !set_up(fluid)) return 2;
        if (!run(fluid, 0, a + b) || !end_of(fluid, whole)) return 3;
    }
    SphStateDigest atSave;
    std::vector<unsigned char> blob;
    {
        SPHFluidGPU fluid(n, /*seed=*/7);
        if (!fluid.LastError().empty() || !set_up(fluid) || !run(fluid, 0, a)) return 2;
        if (!fluid.SaveState(blob) || !fluid.StateDigest(atSave)) return 4;
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size() || std::fclose(f) != 0) { std::printf("cannot write %s\n", path.c_str()); return 4; }
    }                                                                        // the engine is gone
    std::vector<unsigned char> file;
    {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) { std::printf("cannot read %s\n", path.c_str()); return 4; }
        unsigned char buf[65536];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
        std::fclose(f);
    }
    SphStateInfo info;
    if (!SPHFluidGPU::PeekState(file.data(), file.size(), info)) { std::printf("the saved file is refused: %s\n", sph_last_error()); return 7; }
    std::printf("checkpoint after %d substeps: %zu bytes, %llu particles\n", a, file.size(), (unsigned long long)info.n);
    for (int i = 0; i < SPH_STATE_SECTION_COUNT; ++i) {
        if (info.sections & (1u << i)) std::printf("  %-10s %10llu bytes at %llu\n", kNames[i], (unsigned long long)info.bytes[i], (unsigned long long)info.offset[i]);
        if (((info.sections ^ atSave.sections) & (1u << i)) || info.sum[i][0] != atSave.sum[i][0] || info.sum[i][1] != atSave.sum[i][1]) {
            std::printf("section %s: the file's checksum is not the digest taken at the save\n", kNames[i]);
            return 7;
        }
    }
    End resumed;
    {
        SPHFluidGPU fluid(n / 3 + 100, /*seed=*/3);                         // another size, no features: the load makes it the saved engine
        if (!fluid.LastError().empty()) return 2;
        const size_t spots[5] = {41, 250, 300, file.size() / 2, file.size() - 1};
        for (size_t at : spots) {                                           // one flipped byte anywhere: refused, by the parser and by the load
            std::vector<unsigned char> bad(file);
            bad[at] ^= 0x20;
            SphStateInfo scratch;
            if (SPHFluidGPU::PeekState(bad.data(), bad.size(), scratch) || sph_state_load(fluid.Handle(), bad.data(), bad.size()) == SPH_OK) {
                std::printf("a blob with byte %zu flipped is accepted\n", at);
                return 8;
            }
        }
        if (!fluid.LoadState(file.data(), file.size())) return 5;
        if (!run(fluid, a, b) || !end_of(fluid, resumed)) return 3;
    }
    print_digest("uninterrupted:", whole.digest);
    print_digest("saved, loaded and continued:", resumed.digest);
    if (std::memcmp(&whole.digest, &resumed.digest, sizeof(SphStateDigest)) != 0) { std::printf("the digests differ\n"); return 6; }
    if (whole.records.size() != resumed.records.size() || std::memcmp(whole.records.data(), resumed.records.data(), whole.records.size() * sizeof(SPHParticle)) != 0 ||
        whole.tracers.size() != resumed.tracers.size() || std::memcmp(whole.tracers.data(), resumed.tracers.data(), whole.tracers.size() * sizeof(SphTracer)) != 0 ||
        whole.books.size() != resumed.books.size() || std::memcmp(whole.books.data(), resumed.books.data(), whole.books.size() * sizeof(SphGateBooks)) != 0 ||
        whole.bodies.size() != resumed.bodies.size() || std::memcmp(whole.bodies.data(), resumed.bodies.data(), whole.bodies.size() * sizeof(SphObstacle)) != 0 ||
        whole.substeps != resumed.substeps || std::memcmp(&whole.time, &resumed.time, sizeof(double)) != 0) {
        std::printf("the two ends differ\n");
        return 9;
    }
    std::printf("checkpoint_resume OK\n");
    return 0;
}
