// SPHFluidGPU_hip.hpp -- header-only C++17 twin of the reference class `SPHFluidGPU`
// (/root/reference/ComponentFramework/SPHFluid3D.h:26-210) on top of the C-ABI in sph_abi.h.
//
// Scene0p-style code compiles against this header unchanged for the hot path: same class
// name, same public member names (`param_*`, `numParticles`, `particles`, `gridSizeX/Y/Z`,
// `numCells`, `gridMinV`, `cellSize`, `box`), same method names and argument meaning
// (`DispatchCompute`, `ResetSimulation`, `ApplyWaveImpulse`, `EffectiveHalf`,
// `ComputeGridExtents`, `GetNumFluids`, `GetFluidVBO`).  The GL object ids Scene0p touches on the
// simulation side (`ssbo`, `GetFluidVBO()`) and the dead `riverMode` switch exist as INERT members
// (0 / false) so that those lines compile unchanged; there is no GL buffer behind them: renderers
// take the device pointer from DeviceParticles() or a packed buffer from PackRenderBuffer()
// instead.  Error convention as the reference: methods return void and log
// (Debug::FatalError only logs, Debug.cpp:54); LastError() exposes the message.
//
// If the host project has MATH::Vec3 / Vec4 (its "MathLibrary"), define
// SPH_HIP_HAVE_MATHLIB before including this header; otherwise minimal PODs are provided.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sph_abi.h"

#ifndef SPH_HIP_HAVE_MATHLIB
namespace MATH {
struct Vec3 {
    float x = 0, y = 0, z = 0;
    Vec3() = default;
    Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
struct Vec4 {
    float x = 0, y = 0, z = 0, w = 0;
    Vec4() = default;
    Vec4(float x_, float y_, float z_, float w_) : x(x_), y(y_), z(z_), w(w_) {}
};
}  // namespace MATH
#endif

struct SPHParticle {              // SPHFluid3D.h:12-24, layout-identical to SphParticle
    MATH::Vec4 pos, vel, acc;
    float density, pressure, padA, padB;
    int isGhost, isActive, padC, pad0;
};
static_assert(sizeof(SPHParticle) == sizeof(SphParticle), "SPHParticle must stay 80 bytes");

class SPHFluidGPU {
public:
    explicit SPHFluidGPU(size_t numParticles_, uint32_t seed_ = 1, void* hipStream = nullptr)
        : numParticles(numParticles_), seed(seed_), stream(hipStream) {
        SphParams p;
        sph_params_default(&p);
        FromParams(p);
        Create();
    }
    ~SPHFluidGPU() { sph_destroy(engine); }
    SPHFluidGPU(const SPHFluidGPU&) = delete;
    SPHFluidGPU& operator=(const SPHFluidGPU&) = delete;

    // ---- methods Scene0p calls (Scene0p.cpp:83,1488,3739,1457,3623,1094,1467,2575,655) ----
    void DispatchCompute(float overrideDt = -1.0f) {                    // SPHFluid3D.cpp:431
        SphParams p = ToParams();                                       // members are re-read every dispatch (:458-506)
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return;
        SphFountain f{fountainMode ? 1 : 0, {fountainOffset.x, fountainOffset.y, fountainOffset.z}, fountainRadius, fountainSpread,
                      fountainJetSpeedLive, fountainDrainLevel, fountainDrainPerSec, fountainSeed};
        if (Check(sph_set_fountain(engine, &f), "sph_set_fountain")) return;
        if (PushRiver()) return;                                        // river members, step 5 (:511-516)
        if (Check(sph_dispatch(engine, overrideDt), "sph_dispatch")) return;
        if (fountainMode && !riverMode && !param_pause) ++fountainSeed; // glUniform1ui("uSeed", fountainSeed++), :541 (fountain step only `!riverMode`, :519)
        RefreshGrid();
    }
    void SimulateSubstep(float overrideDt = -1.0f) { DispatchCompute(overrideDt); }   // BASELINE.json's name
    void ResetSimulation() {                                            // SPHFluid3D.cpp:713
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return;
        if (PushRiver()) return;                                        // riverMode && !terrainHeights.empty() selects the spawn branch (:104)
        surface = SphSurface{};
        if (Check(sph_reset(engine, numParticles, seed), "sph_reset")) return;
        AfterSpawn();
        std::printf("Reset: particles=%zu fluids=%zu grid=%dx%dx%d cells=%d\n", particles.size(), numFluids, gridSizeX, gridSizeY, gridSizeZ, numCells);
    }
    void ApplyWaveImpulse(float amplitude, float wavelength, float phase, const MATH::Vec3& dir,
                          float yMin = -FLT_MAX, float yMax = FLT_MAX) {   // SPHFluid3D.cpp:604
        const float d[3] = {dir.x, dir.y, dir.z};
        Check(sph_apply_wave_impulse(engine, amplitude, wavelength, phase, d, yMin, yMax), "sph_apply_wave_impulse");
    }
    void ApplyVortexImpulse(float tangentKick, float inwardKick) {       // SPHFluid3D.cpp:627
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return;
        Check(sph_apply_vortex_impulse(engine, tangentKick, inwardKick), "sph_apply_vortex_impulse");
    }
    void ApplyAttractorImpulse(const MATH::Vec3& point, float pullKick, float radius) {   // SPHFluid3D.cpp:650
        const float q[3] = {point.x, point.y, point.z};
        Check(sph_apply_attractor_impulse(engine, q, pullKick, radius), "sph_apply_attractor_impulse");
    }
    void ApplyCurlFlow(float kick, float scale, float time) {            // SPHFluid3D.cpp:668
        Check(sph_apply_curl_flow(engine, kick, scale, time), "sph_apply_curl_flow");
    }
    void SetStencilTargets(const std::vector<MATH::Vec4>& points) {      // SPHFluid3D.cpp:684
        stencilCount = int(points.size());
        Check(sph_set_stencil_targets(engine, points.empty() ? nullptr : &points[0].x, points.size()), "sph_set_stencil_targets");
    }
    void ApplyStencilAttract(float pullKick, float dampKick) {           // SPHFluid3D.cpp:695
        Check(sph_apply_stencil_attract(engine, pullKick, dampKick), "sph_apply_stencil_attract");
    }
    void GenerateRiverTerrain(int seed_) {                               // SPHFluid3D.cpp:772-878 (heightfield upload = sph_set_river)
        SphParams p = ToParams();
        SphRiver r = ToRiver();
        terrainHeights.assign(size_t(terrainW) * size_t(terrainH), 0.0f);
        if (Check(sph_generate_river_terrain(&p, seed_, &r, terrainHeights.data()), "sph_generate_river_terrain")) return;
        param_gravityY = p.param_gravityY; param_gravityZ = p.param_gravityZ;   // :864-865
        terrainWorldMinX = r.terrainWorldMinX; terrainWorldMinZ = r.terrainWorldMinZ;
        terrainWorldSizeX = r.terrainWorldSizeX; terrainWorldSizeZ = r.terrainWorldSizeZ;
        riverEmitterPos = MATH::Vec3(r.riverEmitterPos[0], r.riverEmitterPos[1], r.riverEmitterPos[2]);
        riverEmitterVel = MATH::Vec3(r.riverEmitterVel[0], r.riverEmitterVel[1], r.riverEmitterVel[2]);
        riverEmitterRadius = r.riverEmitterRadius; riverSinkY = r.riverSinkY; riverSinkZMax = r.riverSinkZMax;
        riverAmp = r.riverAmp; riverFreq = r.riverFreq; riverPhase = r.riverPhase;
        riverChannelWidth = r.riverChannelWidth; riverChannelDepth = r.riverChannelDepth; riverSlopeDrop = r.riverSlopeDrop;
        terrainDirty = true;
        std::printf("[River] seed=%d amp=%g freq=%g width=%g slope=%g\n", seed_, riverAmp, riverFreq, riverChannelWidth, riverSlopeDrop);
    }
    int stencilCount = 0;                                                // SPHFluid3D.h:55
    MATH::Vec3 EffectiveHalf() const {                                  // SPHFluid3D.h:127
        SphParams p = ToParams();
        float h[3];
        sph_effective_half(&p, h);
        return MATH::Vec3(h[0], h[1], h[2]);
    }
    void ComputeGridExtents() {                                         // SPHFluid3D.cpp:354
        SphParams p = ToParams();
        SphGridInfo g;
        sph_compute_grid_extents(&p, &g);
        SetGrid(g);
    }
    size_t GetNumFluids() const { return numFluids; }                   // SPHFluid3D.cpp:601
    // SPHFluid3D.h:37; Scene0p.cpp:85,1459,3625 only store the id.  Inert: no GL object exists (0 = "no buffer").
    unsigned int GetFluidVBO() const { return 0u; }

    // ---- what replaces the GL buffer ids -------------------------------------------------
    const SPHParticle* DeviceParticles() {     // device pointer of the 80-byte array in original order (the `ssbo`)
        const SphParticle* p = nullptr;
        Check(sph_device_particles(engine, &p), "sph_device_particles");
        return reinterpret_cast<const SPHParticle*>(p);
    }
    // packed (x, y, z, w) per particle in original order into a device buffer of the renderer (w: 0 one, 1 density,
    // 2 foam, 3 speed, 4 dye): the render-side replacement of binding 0 reads (fluidDepth.vert, particleImpostor.vert)
    void PackRenderBuffer(float* devOut4, int wMode = 0) { Check(sph_pack_render_buffer(engine, devOut4, sph_num_particles(engine), wMode), "sph_pack_render_buffer"); }
    // Field sampling (engine extension, sph_abi.h "field sampling"): the fields of the current state at probe points (host
    // vectors; synchronises) or on a lattice origin + i * spacing, x fastest, into a device buffer (asynchronous).  Members are
    // pushed first, as DispatchCompute does.  Returns false on error (LastError()).
    bool SamplePoints(const std::vector<MATH::Vec4>& points, std::vector<SphSample>& out) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        out.resize(points.size());
        return !Check(sph_sample_points(engine, points.empty() ? nullptr : &points[0].x, points.size(), out.empty() ? nullptr : out.data()),
                      "sph_sample_points");
    }
    bool SampleLattice(const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], int field, void* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        return !Check(sph_sample_lattice(engine, o, s, dims, field, devOut), "sph_sample_lattice");
    }
    // Neighbour lists (engine extension, sph_abi.h "fixed-radius neighbour lists"): CSR lists of the particles within
    // `radius` (<= 0: param_h; at most three cells) of every particle (rows numbered by particle id) or of query points in DEVICE memory
    // (4 floats each), in the engine's order.  flags: SPH_NEIGHBORS_SELF / _HALF / _COUNT_ONLY; maxPairs > 0 refuses larger lists.  The
    // lists stay in the engine until the next call, ResetSimulation or the destructor; DownloadNeighbors copies them to the host
    // (indices stays empty for count-only lists).  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    bool Neighbors(SphNeighborInfo& out, float radius = 0.0f, int flags = 0, uint64_t maxPairs = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_neighbors_build(engine, radius > 0.0f ? radius : param_h, flags, maxPairs, &out), "sph_neighbors_build");
    }
    bool QueryNeighbors(const float* devPoints4, size_t m, float radius, SphNeighborInfo& out, int flags = 0, uint64_t maxPairs = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_neighbors_query(engine, devPoints4, m, radius, flags, maxPairs, &out), "sph_neighbors_query");
    }
    SphNeighborInfo NeighborInfo() {
        SphNeighborInfo info{};
        Check(sph_neighbors_info(engine, &info), "sph_neighbors_info");
        return info;
    }
    bool DownloadNeighbors(std::vector<int64_t>& offsets, std::vector<int32_t>& indices) {
        const SphNeighborInfo info = NeighborInfo();
        const int64_t* dOff = nullptr;
        const int32_t* dIdx = nullptr;
        if (Check(sph_neighbors_device(engine, &dOff, &dIdx), "sph_neighbors_device")) return false;
        offsets.assign(size_t(info.rows) + 1, 0);
        indices.assign(dIdx ? size_t(info.total) : 0, 0);
        return !Check(sph_neighbors_download(engine, offsets.data(), dIdx ? indices.data() : nullptr, indices.size()), "sph_neighbors_download");
    }
    // Connected components (engine extension, sph_abi.h "connected components"): which particles hang together under
    // the neighbour relation at `radius` (<= 0: param_h; at most three cells).  flags: SPH_COMPONENTS_FLUID_ONLY.  The result stays in the
    // engine until the next call, ResetSimulation or the destructor; DownloadComponents copies labels[n], roots[n] and the table of one
    // row per body to the host.  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    bool Components(SphComponentInfo& out, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_components_build(engine, radius > 0.0f ? radius : param_h, flags, &out), "sph_components_build");
    }
    SphComponentInfo ComponentInfo() {
        SphComponentInfo info{};
        Check(sph_components_info(engine, &info), "sph_components_info");
        return info;
    }
    bool DownloadComponents(std::vector<int32_t>& labels, std::vector<int32_t>& roots, std::vector<SphComponent>& table) {
        SphComponentInfo info{};
        if (Check(sph_components_info(engine, &info), "sph_components_info")) return false;
        labels.assign(size_t(info.rows), 0);
        roots.assign(size_t(info.rows), 0);
        table.assign(size_t(info.numComponents), SphComponent{});
        return !Check(sph_components_download(engine, labels.empty() ? nullptr : labels.data(), roots.empty() ? nullptr : roots.data(),
                                              table.empty() ? nullptr : table.data(), table.size()), "sph_components_download");
    }
    // k nearest neighbours (engine extension, sph_abi.h "k nearest neighbours"): per particle (rows numbered by
    // particle id) or per query point in DEVICE memory (4 floats each) the k nearest particles within `radius` (<= 0: param_h; at most
    // three cells), nearest first, ties to the smaller id.  flags: SPH_KNN_SELF / _FLUID_ONLY; 1 <= k <= SPH_KNN_MAX_K.  The rows stay in
    // the engine until the next call, ResetSimulation or the destructor; DownloadKnn copies indices[rows * k] (padded with -1),
    // dist2[rows * k] (padded with +inf) and counts[rows] to the host.  Members are pushed first, as DispatchCompute does.  Return false
    // on error (LastError()).
    bool Knn(SphKnnInfo& out, int k, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_knn_build(engine, k, radius > 0.0f ? radius : param_h, flags, &out), "sph_knn_build");
    }
    bool QueryKnn(const float* devPoints4, size_t m, int k, float radius, SphKnnInfo& out, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_knn_query(engine, devPoints4, m, k, radius, flags, &out), "sph_knn_query");
    }
    SphKnnInfo KnnInfo() {
        SphKnnInfo info{};
        Check(sph_knn_info(engine, &info), "sph_knn_info");
        return info;
    }
    bool DownloadKnn(std::vector<int32_t>& indices, std::vector<float>& dist2, std::vector<uint32_t>& counts) {
        SphKnnInfo info{};
        if (Check(sph_knn_info(engine, &info), "sph_knn_info")) return false;
        indices.assign(size_t(info.rows) * size_t(info.k), 0);
        dist2.assign(indices.size(), 0.0f);
        counts.assign(size_t(info.rows), 0u);
        return !Check(sph_knn_download(engine, indices.empty() ? nullptr : indices.data(), dist2.empty() ? nullptr : dist2.data(),
                                       counts.empty() ? nullptr : counts.data()), "sph_knn_download");
    }
    // Free-surface particles (engine extension, sph_abi.h "free-surface particles"): per particle (rows numbered by
    // particle id) or per query point in DEVICE memory (4 floats each) whether it lies in the outer shell of the fluid, the outward normal
    // there, the offset of the neighbours' weighted centroid in units of the radius, and -- particle rows -- the crest measure of the shell's
    // convexity; from the positions alone.  cfg: sph_shell_default's fields (radius <= 0: param_h; at most three cells).  The rows stay in
    // the engine until the next call, ResetSimulation or the destructor; DownloadShell copies rows[rows] and ids[numShell] (the shell's
    // rows, ascending) to the host.  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    static SphShellConfig ShellConfig() {
        SphShellConfig cfg;
        sph_shell_default(&cfg);
        return cfg;
    }
    bool Shell(SphShellInfo& out, const SphShellConfig& cfg) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_shell_build(engine, &cfg, &out), "sph_shell_build");
    }
    bool QueryShell(const float* devPoints4, size_t m, const SphShellConfig& cfg, SphShellInfo& out) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_shell_query(engine, devPoints4, m, &cfg, &out), "sph_shell_query");
    }
    SphShellInfo ShellInfo() {
        SphShellInfo info{};
        Check(sph_shell_info(engine, &info), "sph_shell_info");
        return info;
    }
    bool DownloadShell(std::vector<SphShell>& rows, std::vector<int32_t>& ids) {
        SphShellInfo info{};
        if (Check(sph_shell_info(engine, &info), "sph_shell_info")) return false;
        rows.assign(size_t(info.rows), SphShell{});
        ids.assign(size_t(info.numShell), 0);
        return !Check(sph_shell_download(engine, rows.empty() ? nullptr : rows.data(), ids.empty() ? nullptr : ids.data()), "sph_shell_download");
    }
    // Anisotropic kernels (engine extension, sph_abi.h "anisotropic kernels"): per particle (rows numbered by
    // particle id) a smoothed centre and the three semi-axis vectors of an ellipsoid shaped by the neighbourhood, and the lattice of the
    // anisotropic fraction summed from those ellipsoids with its iso-surface.  cfg: sph_aniso_default's fields (radius <= 0: 2 param_h,
    // support <= 0: param_h).  The rows stay in the engine until the next of these calls, ResetSimulation or the destructor;
    // DownloadAniso copies them to the host.  AnisoLattice writes dims[0] * dims[1] * dims[2] floats (x fastest) to DEVICE memory;
    // ExtractAnisoSurface meshes that lattice as ExtractSurface meshes a field (DownloadSurface copies the result).  Members are pushed
    // first, as DispatchCompute does.  Return false on error (LastError()).
    static SphAnisoConfig AnisoConfig() {
        SphAnisoConfig cfg;
        sph_aniso_default(&cfg);
        return cfg;
    }
    bool Anisotropy(SphAnisoInfo& out, const SphAnisoConfig& cfg) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aniso_build(engine, &cfg, &out), "sph_aniso_build");
    }
    SphAnisoInfo AnisoInfo() {
        SphAnisoInfo info{};
        Check(sph_aniso_info(engine, &info), "sph_aniso_info");
        return info;
    }
    bool DownloadAniso(std::vector<SphAniso>& rows) {
        SphAnisoInfo info{};
        if (Check(sph_aniso_info(engine, &info), "sph_aniso_info")) return false;
        rows.assign(size_t(info.rows), SphAniso{});
        return !Check(sph_aniso_download(engine, rows.empty() ? nullptr : rows.data()), "sph_aniso_download");
    }
    bool AnisoLattice(const SphAnisoConfig& cfg, const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        SphAnisoInfo info{};
        return !Check(sph_aniso_lattice(engine, &cfg, o, s, dims, devOut, &info), "sph_aniso_lattice");
    }
    bool ExtractAnisoSurface(const SphAnisoConfig& cfg, const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], float iso, SphSurface& out) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        SphAnisoInfo info{};
        surface = SphSurface{};
        if (Check(sph_aniso_surface(engine, &cfg, o, s, dims, iso, &out, &info), "sph_aniso_surface")) return false;
        surface = out;
        return true;
    }
    // Fused neighbourhood reductions (engine extension, sph_abi.h "fused neighbourhood reductions"): sum, mean, max
    // or min of the caller's devValues[n][channels] over the neighbours of every particle (rows numbered by particle id) or of m query
    // points, written to devOut[rows][planes][channels] and, where not null, devCount[rows]; all three are DEVICE memory.  cfg:
    // sph_aggregate_default's fields with radius set (AggregateConfig: param_h).  The engine keeps nothing and does not synchronise: the
    // results are complete after Sync().  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    SphAggregateConfig AggregateConfig() const {
        SphAggregateConfig cfg;
        sph_aggregate_default(&cfg);
        cfg.radius = param_h;
        return cfg;
    }
    bool Aggregate(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devValues, float* devOut, uint32_t* devCount = nullptr) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_particles(engine, &cfg, devValues, devOut, devCount, &out), "sph_aggregate_particles");
    }
    bool QueryAggregate(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                        uint32_t* devCount = nullptr) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_query(engine, &cfg, devPoints4, m, devValues, devOut, devCount, &out), "sph_aggregate_query");
    }
    // The same for HOST arrays (values n * channels floats; points4 m * 4 floats or null for particle targets): out is sized to rows *
    // planes * channels, counts (may be null) to rows.  Synchronises.
    bool Aggregate(SphAggregateInfo& info, const SphAggregateConfig& cfg, const std::vector<float>& values, std::vector<float>& out,
                   std::vector<uint32_t>* counts = nullptr, const float* points4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t rows = points4 ? m : sph_num_particles(engine), planes = (cfg.flags & SPH_AGGREGATE_MOMENTS) ? 4 : 1;
        if (cfg.channels < 1 || values.size() != sph_num_particles(engine) * size_t(cfg.channels)) return !Check(SPH_ERR_ARG, "Aggregate: values.size() is not n * channels");
        out.assign(rows * planes * size_t(cfg.channels), 0.0f);
        if (counts) counts->assign(rows, 0u);
        return !Check(sph_aggregate_staged(engine, &cfg, points4, m, values.data(), out.data(), counts ? counts->data() : nullptr, &info), "sph_aggregate_staged");
    }
    // The adjoint of those sums (sph_abi.h "the adjoint of the neighbourhood sums"), cfg.op SUM: devG[rows][planes]
    // [channels] is what Aggregate / QueryAggregate would write, devOut[n][channels] by particle id what each particle sums over the rows
    // that accept it.  QueryAggregateAdjoint is the point -> particle transfer.  DEVICE memory, no synchronisation, as Aggregate.
    bool AggregateAdjoint(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devG, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_adjoint_particles(engine, &cfg, devG, devOut, &out), "sph_aggregate_adjoint_particles");
    }
    bool QueryAggregateAdjoint(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devPoints4, size_t m, const float* devG, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_adjoint_query(engine, &cfg, devPoints4, m, devG, devOut, &out), "sph_aggregate_adjoint_query");
    }
    // The same for HOST arrays (g rows * planes * channels floats; points4 m * 4 floats or null for particle targets): out is sized to
    // n * channels.  Synchronises.
    bool AggregateAdjoint(SphAggregateInfo& info, const SphAggregateConfig& cfg, const std::vector<float>& g, std::vector<float>& out,
                          const float* points4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine), rows = points4 ? m : n, planes = (cfg.flags & SPH_AGGREGATE_MOMENTS) ? 4 : 1;
        if (cfg.channels < 1 || g.size() != rows * planes * size_t(cfg.channels)) return !Check(SPH_ERR_ARG, "AggregateAdjoint: g.size() is not rows * planes * channels");
        out.assign(n * size_t(cfg.channels), 0.0f);
        return !Check(sph_aggregate_adjoint_staged(engine, &cfg, points4, m, g.data(), out.data(), &info), "sph_aggregate_adjoint_staged");
    }
    // MAX / MIN with the winners (devArg int32[rows][channels]: the smallest id that holds the extremum, -1 for none; devPoints4 null:
    // particle targets) and the routing of devG[rows][channels] through them into devOut[n][channels].  DEVICE memory, no synchronisation.
    bool AggregateArg(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devValues, float* devOut, uint32_t* devCount, int32_t* devArg,
                      const float* devPoints4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        if (devPoints4) return !Check(sph_aggregate_arg_query(engine, &cfg, devPoints4, m, devValues, devOut, devCount, devArg, &out), "sph_aggregate_arg_query");
        return !Check(sph_aggregate_arg_particles(engine, &cfg, devValues, devOut, devCount, devArg, &out), "sph_aggregate_arg_particles");
    }
    bool AggregateRoute(SphAggregateInfo& out, const SphAggregateConfig& cfg, const int32_t* devArg, const float* devG, float* devOut,
                        const float* devPoints4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        if (devPoints4) return !Check(sph_aggregate_route_query(engine, &cfg, devPoints4, m, devArg, devG, devOut, &out), "sph_aggregate_route_query");
        return !Check(sph_aggregate_route_particles(engine, &cfg, devArg, devG, devOut, &out), "sph_aggregate_route_particles");
    }
    // Position gradients of the neighbourhood sums (sph_abi.h "position gradients of the neighbourhood sums"): with
    // L = sum devG . Aggregate(devValues) under cfg (op SUM), devOut[n][3] = dL/dx of the particles; for query targets devOutPoints[m][3]
    // and devOutParticles[n][3], either of which may be null (its walk is not launched).  DEVICE memory, no synchronisation, as Aggregate.
    bool AggregatePositionGrad(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devValues, const float* devG, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_posgrad_particles(engine, &cfg, devValues, devG, devOut, &out), "sph_aggregate_posgrad_particles");
    }
    bool QueryAggregatePositionGrad(SphAggregateInfo& out, const SphAggregateConfig& cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                    float* devOutPoints, float* devOutParticles) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_posgrad_query(engine, &cfg, devPoints4, m, devValues, devG, devOutPoints, devOutParticles, &out), "sph_aggregate_posgrad_query");
    }
    // The same for HOST arrays (values n * channels floats, g rows * planes * channels): grad is sized to n * 3.  Synchronises.
    bool AggregatePositionGrad(SphAggregateInfo& info, const SphAggregateConfig& cfg, const std::vector<float>& values, const std::vector<float>& g,
                               std::vector<float>& grad) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine), planes = (cfg.flags & SPH_AGGREGATE_MOMENTS) ? 4 : 1;
        if (cfg.channels < 1 || values.size() != n * size_t(cfg.channels) || g.size() != n * planes * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "AggregatePositionGrad: values.size() is not n * channels or g.size() is not n * planes * channels");
        grad.assign(n * 3, 0.0f);
        return !Check(sph_aggregate_posgrad_staged(engine, &cfg, nullptr, 0, values.data(), g.data(), nullptr, grad.data(), &info), "sph_aggregate_posgrad_staged");
    }
    // points4: m * 4 floats; gradPoints is sized to m * 3 and gradParticles to n * 3.
    bool QueryAggregatePositionGrad(SphAggregateInfo& info, const SphAggregateConfig& cfg, const float* points4, size_t m, const std::vector<float>& values,
                                    const std::vector<float>& g, std::vector<float>& gradPoints, std::vector<float>& gradParticles) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine), planes = (cfg.flags & SPH_AGGREGATE_MOMENTS) ? 4 : 1;
        if (!points4 || cfg.channels < 1 || values.size() != n * size_t(cfg.channels) || g.size() != m * planes * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "QueryAggregatePositionGrad: null points, values.size() is not n * channels or g.size() is not m * planes * channels");
        gradPoints.assign(m * 3 + 1, 0.0f);                            // (one spare float: the pointer of an empty result must not be null)
        gradParticles.assign(n * 3 + 1, 0.0f);
        const bool ok = !Check(sph_aggregate_posgrad_staged(engine, &cfg, points4, m, values.data(), g.data(), gradPoints.data(), gradParticles.data(), &info),
                               "sph_aggregate_posgrad_staged");
        gradPoints.resize(m * 3);
        gradParticles.resize(n * 3);
        return ok;
    }
    // Filter-grid basis sums (sph_abi.h "filter-grid basis sums"): devOut[rows][K^3][channels] = the sums of
    // w * phi_b(x_j - x_i) * devValues[j][c] over the neighbours, the linear part of a continuous convolution (the caller multiplies by
    // the filters), and the exact transpose devH[rows][K^3][channels] -> devOut[n][channels].  cfg: sph_aggregate_basis_default's fields
    // with radius set (BasisConfig: param_h).  DEVICE memory, no synchronisation, as Aggregate.
    SphBasisConfig BasisConfig() const {
        SphBasisConfig cfg;
        sph_aggregate_basis_default(&cfg);
        cfg.radius = param_h;
        return cfg;
    }
    bool AggregateBasis(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devValues, float* devOut, uint32_t* devCount = nullptr) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_particles(engine, &cfg, devValues, devOut, devCount, &out), "sph_aggregate_basis_particles");
    }
    bool QueryAggregateBasis(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                             uint32_t* devCount = nullptr) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_query(engine, &cfg, devPoints4, m, devValues, devOut, devCount, &out), "sph_aggregate_basis_query");
    }
    bool AggregateBasisAdjoint(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devH, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_adjoint_particles(engine, &cfg, devH, devOut, &out), "sph_aggregate_basis_adjoint_particles");
    }
    bool QueryAggregateBasisAdjoint(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devPoints4, size_t m, const float* devH, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_adjoint_query(engine, &cfg, devPoints4, m, devH, devOut, &out), "sph_aggregate_basis_adjoint_query");
    }
    // The same for HOST arrays (points4 m * 4 floats, or null for particle targets): out is sized by the call.  Synchronises.
    bool AggregateBasis(SphAggregateInfo& info, const SphBasisConfig& cfg, const std::vector<float>& values, std::vector<float>& out,
                        std::vector<uint32_t>* counts = nullptr, const float* points4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t rows = points4 ? m : sph_num_particles(engine);
        if (cfg.channels < 1 || cfg.size < 2 || cfg.size > 4 || values.size() != sph_num_particles(engine) * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "AggregateBasis: values.size() is not n * channels, or a bad size");
        out.assign(rows * size_t(cfg.size * cfg.size * cfg.size) * size_t(cfg.channels), 0.0f);
        if (counts) counts->assign(rows, 0u);
        return !Check(sph_aggregate_basis_staged(engine, &cfg, points4, m, values.data(), out.data(), counts ? counts->data() : nullptr, &info), "sph_aggregate_basis_staged");
    }
    bool AggregateBasisAdjoint(SphAggregateInfo& info, const SphBasisConfig& cfg, const std::vector<float>& h, std::vector<float>& out,
                               const float* points4 = nullptr, size_t m = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine), rows = points4 ? m : n;
        if (cfg.channels < 1 || cfg.size < 2 || cfg.size > 4 || h.size() != rows * size_t(cfg.size * cfg.size * cfg.size) * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "AggregateBasisAdjoint: h.size() is not rows * K^3 * channels");
        out.assign(n * size_t(cfg.channels), 0.0f);
        return !Check(sph_aggregate_basis_adjoint_staged(engine, &cfg, points4, m, h.data(), out.data(), &info), "sph_aggregate_basis_adjoint_staged");
    }
    // Position gradients of the basis sums (sph_abi.h "position gradients of the basis sums"): with
    // L = sum devG . AggregateBasis(devValues) under cfg, devG[rows][K^3][channels], devOut[n][3] = dL/dx of the particles; for query targets
    // devOutPoints[m][3] and devOutParticles[n][3], either of which may be null (its walk is not launched).  DEVICE memory, no
    // synchronisation, as Aggregate.
    bool AggregateBasisPositionGrad(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devValues, const float* devG, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_posgrad_particles(engine, &cfg, devValues, devG, devOut, &out), "sph_aggregate_basis_posgrad_particles");
    }
    bool QueryAggregateBasisPositionGrad(SphAggregateInfo& out, const SphBasisConfig& cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                         float* devOutPoints, float* devOutParticles) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_aggregate_basis_posgrad_query(engine, &cfg, devPoints4, m, devValues, devG, devOutPoints, devOutParticles, &out),
                      "sph_aggregate_basis_posgrad_query");
    }
    // The same for HOST arrays (values n * channels floats, g rows * K^3 * channels): grad is sized to n * 3.  Synchronises.
    bool AggregateBasisPositionGrad(SphAggregateInfo& info, const SphBasisConfig& cfg, const std::vector<float>& values, const std::vector<float>& g,
                                    std::vector<float>& grad) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine);
        if (cfg.channels < 1 || cfg.size < 2 || cfg.size > 4 || values.size() != n * size_t(cfg.channels) ||
            g.size() != n * size_t(cfg.size * cfg.size * cfg.size) * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "AggregateBasisPositionGrad: values.size() is not n * channels or g.size() is not n * K^3 * channels");
        grad.assign(n * 3, 0.0f);
        return !Check(sph_aggregate_basis_posgrad_staged(engine, &cfg, nullptr, 0, values.data(), g.data(), nullptr, grad.data(), &info),
                      "sph_aggregate_basis_posgrad_staged");
    }
    // points4: m * 4 floats; gradPoints is sized to m * 3 and gradParticles to n * 3.
    bool QueryAggregateBasisPositionGrad(SphAggregateInfo& info, const SphBasisConfig& cfg, const float* points4, size_t m, const std::vector<float>& values,
                                         const std::vector<float>& g, std::vector<float>& gradPoints, std::vector<float>& gradParticles) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const size_t n = sph_num_particles(engine);
        if (!points4 || cfg.channels < 1 || cfg.size < 2 || cfg.size > 4 || values.size() != n * size_t(cfg.channels) ||
            g.size() != m * size_t(cfg.size * cfg.size * cfg.size) * size_t(cfg.channels))
            return !Check(SPH_ERR_ARG, "QueryAggregateBasisPositionGrad: null points, values.size() is not n * channels or g.size() is not m * K^3 * channels");
        gradPoints.assign(m * 3 + 1, 0.0f);                            // (one spare float: the pointer of an empty result must not be null)
        gradParticles.assign(n * 3 + 1, 0.0f);
        const bool ok = !Check(sph_aggregate_basis_posgrad_staged(engine, &cfg, points4, m, values.data(), g.data(), gradPoints.data(), gradParticles.data(), &info),
                               "sph_aggregate_basis_posgrad_staged");
        gradPoints.resize(m * 3);
        gradParticles.resize(n * 3);
        return ok;
    }
    // Ray casts (engine extension, sph_abi.h "ray casts"): for each of m rays of 8 floats (ox, oy, oz, tmin, dx, dy,
    // dz, tmax; t in units of the given direction) the first particle the ray enters, every particle a solid sphere of `radius` (<= 0:
    // param_h / 4; at most half a cell).  flags: SPH_RAYS_FLUID_ONLY / _ANY_HIT.  CastRays takes host rays, CastRaysDevice rays in DEVICE
    // memory.  The hits stay in the engine until the next call, ResetSimulation or the destructor; DownloadRayHits copies them to the host
    // (a miss is t = +inf, id = -1, the rest 0).  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    bool CastRays(const std::vector<float>& rays8, SphRaysInfo& out, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_rays_cast(engine, rays8.empty() ? nullptr : rays8.data(), rays8.size() / 8, radius > 0.0f ? radius : 0.25f * param_h, flags, &out),
                      "sph_rays_cast");
    }
    bool CastRaysDevice(const float* devRays8, size_t m, SphRaysInfo& out, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_rays_cast_device(engine, devRays8, m, radius > 0.0f ? radius : 0.25f * param_h, flags, &out), "sph_rays_cast_device");
    }
    SphRaysInfo RaysInfo() {
        SphRaysInfo info{};
        Check(sph_rays_info(engine, &info), "sph_rays_info");
        return info;
    }
    bool DownloadRayHits(std::vector<SphRayHit>& hits) {
        SphRaysInfo info{};
        if (Check(sph_rays_info(engine, &info), "sph_rays_info")) return false;
        hits.assign(size_t(info.rays), SphRayHit{});
        return !Check(sph_rays_download(engine, hits.empty() ? nullptr : hits.data()), "sph_rays_download");
    }
    // Ray spans (engine extension, sph_abi.h "ray spans"): for each of m rays what it crosses in all -- the number
    // of spheres with a chord of positive length inside [tmin, tmax] (a sphere around the ray's start counts), the first entry and the
    // last exit with their particle ids, and the summed share of the chords in units of 2^-24 of a diameter (thickness = length * 2 r *
    // 2^-24).  radius and flags as CastRays (SPH_RAYS_ANY_HIT is refused).  The spans stay in the engine, beside the hits of CastRays,
    // until the next call, ResetSimulation or the destructor; nothing crossed is (+inf, -inf, -1, -1, 0).  Return false on error.
    bool SpanRays(const std::vector<float>& rays8, SphRaySpansInfo& out, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_rays_span(engine, rays8.empty() ? nullptr : rays8.data(), rays8.size() / 8, radius > 0.0f ? radius : 0.25f * param_h, flags, &out),
                      "sph_rays_span");
    }
    bool SpanRaysDevice(const float* devRays8, size_t m, SphRaySpansInfo& out, float radius = 0.0f, int flags = 0) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_rays_span_device(engine, devRays8, m, radius > 0.0f ? radius : 0.25f * param_h, flags, &out), "sph_rays_span_device");
    }
    SphRaySpansInfo RaySpansInfo() {
        SphRaySpansInfo info{};
        Check(sph_rays_span_info(engine, &info), "sph_rays_span_info");
        return info;
    }
    bool DownloadRaySpans(std::vector<SphRaySpan>& rows) {
        SphRaySpansInfo info{};
        if (Check(sph_rays_span_info(engine, &info), "sph_rays_span_info")) return false;
        rows.assign(size_t(info.rays), SphRaySpan{});
        return !Check(sph_rays_span_download(engine, rows.empty() ? nullptr : rows.data()), "sph_rays_span_download");
    }
    // Iso-surface (engine extension, sph_abi.h "iso-surface"): the closed triangle mesh of {field >= iso} on the lattice
    // origin + i * spacing (dims >= 2 per axis).  `out` holds counts and device arrays borrowed from the engine, valid until the next
    // ExtractSurface, ResetSimulation or the destructor.  DownloadSurface copies the last surface to the host (3 indices per
    // triangle).  Members are pushed first, as DispatchCompute does.  Return false on error (LastError()).
    bool ExtractSurface(const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], int field, float iso, SphSurface& out) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        surface = SphSurface{};
        if (Check(sph_extract_surface(engine, o, s, dims, field, iso, &out), "sph_extract_surface")) return false;
        surface = out;
        return true;
    }
    bool DownloadSurface(std::vector<SphSurfaceVertex>& vertices, std::vector<uint32_t>& triangles3) {
        vertices.resize(surface.numVertices);
        triangles3.resize(size_t(surface.numTriangles) * 3);
        return !Check(sph_surface_download(engine, vertices.empty() ? nullptr : vertices.data(), vertices.size(),
                                           triangles3.empty() ? nullptr : triangles3.data(), triangles3.size() / 3), "sph_surface_download");
    }
    // State statistics (engine extension, sph_abi.h "statistics"): counts, extrema with ids, fp64 sums in a fixed
    // order, cell occupancy and up to 4 histograms (histograms[k]: bins + 2 slots) of the current state, reduced on the device.
    // Members are pushed first, as DispatchCompute does.  Synchronises.  Returns false on error (LastError()).
    bool Statistics(SphStatistics& out, const std::vector<SphHistogramSpec>& specs = {}, std::vector<std::vector<uint64_t>>* histograms = nullptr) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        size_t words = 0;
        for (const auto& h : specs) words += size_t(h.bins) + 2;
        std::vector<uint64_t> flat(words);
        if (Check(sph_statistics(engine, &out, specs.empty() ? nullptr : specs.data(), int(specs.size()), flat.empty() ? nullptr : flat.data()),
                  "sph_statistics")) return false;
        if (histograms) {
            histograms->clear();
            size_t at = 0;
            for (const auto& h : specs) {
                histograms->emplace_back(flat.begin() + at, flat.begin() + at + h.bins + 2);
                at += size_t(h.bins) + 2;
            }
        }
        return true;
    }
    // Derived numbers of a Statistics result with the CURRENT members (they are not part of the device contract).
    double KineticEnergy(const SphStatistics& s) const { return 0.5 * double(param_mass) * s.sumSpeed2; }
    double PotentialEnergy(const SphStatistics& s) const {
        return -double(param_mass) * (double(param_gravityX) * s.sumPos[0] + double(param_gravityY) * s.sumPos[1] + double(param_gravityZ) * s.sumPos[2]);
    }
    MATH::Vec3 CentreOfMass(const SphStatistics& s) const {
        const double n = s.numCounted ? double(s.numCounted) : 1.0;
        return MATH::Vec3(float(s.sumPos[0] / n), float(s.sumPos[1] / n), float(s.sumPos[2] / n));
    }
    double MeanDensity(const SphStatistics& s) const { return s.numCounted ? s.sumDensity / double(s.numCounted) : 0.0; }
    double StdDensity(const SphStatistics& s) const {
        if (!s.numCounted) return 0.0;
        const double m = s.sumDensity / double(s.numCounted), v = s.sumDensity2 / double(s.numCounted) - m * m;
        return v > 0.0 ? std::sqrt(v) : 0.0;
    }
    double Cfl(const SphStatistics& s) const { return double(s.maxSpeed) * double(param_timeStep) / double(param_h); }
    double SphVolume(const SphStatistics& s) const { return double(param_mass) * s.sumInvDensity; }
    // Passive tracers (engine extension, sph_abi.h "passive tracers"): points (x, y, z, initial age) that every substep from now on
    // advects with the fluid's Shepard velocity, behind the substep's own grid build; `history` snapshots, one every `stride`
    // substeps, are kept on the device.  An empty vector drops the set.  TracerHistory returns the stored snapshots oldest first
    // (snapshot k, tracer i at out4[k * NumTracers() + i]) and the number of the first one.  Return false on error (LastError()).
    bool SetTracers(const std::vector<MATH::Vec4>& points, int integrator = SPH_TRACER_MIDPOINT, uint32_t history = 0, uint32_t stride = 1) {
        return !Check(sph_tracers_set(engine, points.empty() ? nullptr : &points[0].x, points.size(), integrator, history, stride), "sph_tracers_set");
    }
    size_t NumTracers() const { return sph_tracers_count(engine); }
    bool DownloadTracers(std::vector<SphTracer>& out) {
        out.resize(sph_tracers_count(engine));
        return !Check(sph_tracers_download(engine, out.empty() ? nullptr : out.data(), out.size()), "sph_tracers_download");
    }
    bool TracerHistory(std::vector<MATH::Vec4>& out4, uint32_t& snapshots, uint64_t& firstSnapshot) {
        uint32_t n = 0;
        if (Check(sph_tracers_info(engine, nullptr, &n, nullptr), "sph_tracers_info")) return false;
        out4.resize(size_t(n) * sph_tracers_count(engine));
        return !Check(sph_tracers_history(engine, out4.empty() ? nullptr : &out4[0].x, n, &snapshots, &firstSnapshot), "sph_tracers_history");
    }
    // Spray, foam and bubbles (engine extension, sph_abi.h "spray, foam and bubbles"): secondary particles that
    // every substep from now on spawns where the fluid foams, classes, moves, ages and removes on the device.  A config with capacity 0
    // drops the pool; DiffuseConfig() returns the defaults to edit.  Return false on error (LastError()).
    static SphDiffuseConfig DiffuseConfig() { SphDiffuseConfig c; sph_diffuse_default(&c); return c; }
    bool SetDiffuse(const SphDiffuseConfig& config) { return !Check(sph_diffuse_set(engine, &config), "sph_diffuse_set"); }
    bool DownloadDiffuse(std::vector<SphDiffuse>& out) {
        SphDiffuseInfo info;
        if (Check(sph_diffuse_info(engine, &info), "sph_diffuse_info")) return false;
        out.resize(info.alive);
        size_t n = 0;
        if (Check(sph_diffuse_download(engine, out.empty() ? nullptr : out.data(), out.size(), &n), "sph_diffuse_download")) return false;
        out.resize(n);
        return true;
    }
    bool DiffuseInfo(SphDiffuseInfo& out) { return !Check(sph_diffuse_info(engine, &out), "sph_diffuse_info"); }
    // Births at wave crests (sph_abi.h "births at wave crests"): the pool's optional second birth term, from a free-surface pass inside
    // the substep.  Needs a pool; a config with rate 0 switches the term off; DiffuseCrest() returns the defaults to edit.  The members
    // are pushed first (the radius is checked against their grid).
    static SphDiffuseCrest DiffuseCrest() { SphDiffuseCrest c; sph_diffuse_crest_default(&c); return c; }
    bool SetDiffuseCrest(const SphDiffuseCrest& crest) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_diffuse_set_crest(engine, &crest), "sph_diffuse_set_crest");
    }
    bool GetDiffuseCrest(SphDiffuseCrest& out) { return !Check(sph_diffuse_get_crest(engine, &out), "sph_diffuse_get_crest"); }
    bool DiffuseCrestInfo(SphDiffuseCrestInfo& out) { return !Check(sph_diffuse_crest_info(engine, &out), "sph_diffuse_crest_info"); }
    // Diffusing scalar channels (engine extension, sph_abi.h "diffusing scalar fields"): K <= SPH_MAX_SCALAR_CHANNELS
    // floats per particle, particle-major in the caller's order, that move with their particles and diffuse between neighbours inside
    // every substep from now on.  values empty: channel 0 is seeded from padB (the dye), the others with 0; channels == 0 drops the set.
    // coeffs: D_0 .. D_{K-1}, then lambda_0 .. lambda_{K-1}.  ScalarMoments and SampleScalarLattice push the members first, as
    // DispatchCompute does.  Return false on error (LastError()).
    bool SetScalars(const std::vector<float>& values, int channels, const std::vector<float>& coeffs) {
        if (channels > 0 && coeffs.size() != size_t(2 * channels)) { lastError = "SetScalars: coeffs must hold 2 * channels floats"; return false; }
        if (!values.empty() && values.size() != sph_num_particles(engine) * size_t(channels)) { lastError = "SetScalars: values must hold numParticles * channels floats"; return false; }
        return !Check(sph_scalars_set(engine, values.empty() ? nullptr : values.data(), sph_num_particles(engine), channels, coeffs.empty() ? nullptr : coeffs.data()),
                      "sph_scalars_set");
    }
    bool SetScalarCoefficients(const std::vector<float>& coeffs) {
        if (coeffs.size() != size_t(2 * sph_scalars_channels(engine))) { lastError = "SetScalarCoefficients: coeffs must hold 2 * channels floats"; return false; }
        return !Check(sph_scalars_set_coefficients(engine, coeffs.data()), "sph_scalars_set_coefficients");
    }
    int NumScalarChannels() const { return sph_scalars_channels(engine); }
    bool DownloadScalars(std::vector<float>& out) {
        out.resize(sph_num_particles(engine) * size_t(sph_scalars_channels(engine)));
        return !Check(sph_scalars_download(engine, out.empty() ? nullptr : out.data(), out.size()), "sph_scalars_download");
    }
    bool PaintScalar(const MATH::Vec3& center, float radius, int channel, float value, int mode = SPH_SCALAR_SET) {
        const float c[3] = {center.x, center.y, center.z};
        return !Check(sph_scalars_paint(engine, c, radius, channel, value, mode), "sph_scalars_paint");
    }
    bool ScalarMoments(std::vector<SphScalarMoments>& out) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        out.assign(SPH_MAX_SCALAR_CHANNELS, SphScalarMoments{});
        if (Check(sph_scalars_moments(engine, out.data()), "sph_scalars_moments")) return false;
        out.resize(size_t(sph_scalars_channels(engine)));
        return true;
    }
    static double ScalarVariance(const SphScalarMoments& m) {
        if (!m.count) return 0.0;
        const double mean = m.sum / double(m.count), v = m.sumSquares / double(m.count) - mean * mean;
        return v > 0.0 ? v : 0.0;
    }
    bool ScalarInfo(uint64_t& substeps, float& maxNumber) { return !Check(sph_scalars_info(engine, &substeps, &maxNumber), "sph_scalars_info"); }
    bool SampleScalarLattice(const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], int channel, float* devOut) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        return !Check(sph_scalars_sample_lattice(engine, o, s, dims, channel, devOut), "sph_scalars_sample_lattice");
    }
    // Active scalars (engine extension, sph_abi.h "active scalars"): SetScalarBuoyancy gives every channel a
    // beta and a reference value (empty vectors switch the kick off), SetScalarSources replaces the table of continuous sources (up to
    // SPH_MAX_SCALAR_SOURCES, an empty vector clears it); both act inside every substep and do not synchronise.  ScalarInjected reads
    // the books per source (fp64 sum of c' - c and the hits) and synchronises.  Return false on error (LastError()).
    bool SetScalarBuoyancy(const std::vector<float>& beta, const std::vector<float>& ref) {
        const size_t k = size_t(sph_scalars_channels(engine));
        if (beta.size() != ref.size() || (!beta.empty() && beta.size() != k)) { lastError = "SetScalarBuoyancy: beta and ref must hold one float per channel"; return false; }
        return !Check(sph_scalars_set_buoyancy(engine, beta.empty() ? nullptr : beta.data(), ref.empty() ? nullptr : ref.data()), "sph_scalars_set_buoyancy");
    }
    bool SetScalarSources(const std::vector<SphScalarSource>& sources) {
        return !Check(sph_scalars_set_sources(engine, sources.empty() ? nullptr : sources.data(), int(sources.size())), "sph_scalars_set_sources");
    }
    bool ScalarInjected(std::vector<double>& sums, std::vector<uint64_t>& hits, double& time, uint64_t& substeps, bool reset = false) {
        sums.assign(SPH_MAX_SCALAR_SOURCES, 0.0);
        hits.assign(SPH_MAX_SCALAR_SOURCES, 0);
        int count = 0;
        SphScalarSource cur[SPH_MAX_SCALAR_SOURCES];
        if (Check(sph_scalars_get_sources(engine, cur, SPH_MAX_SCALAR_SOURCES, &count), "sph_scalars_get_sources")) return false;
        if (Check(sph_scalars_injected(engine, sums.data(), hits.data(), SPH_MAX_SCALAR_SOURCES, &time, &substeps, reset ? 1 : 0), "sph_scalars_injected")) return false;
        sums.resize(size_t(count));
        hits.resize(size_t(count));
        return true;
    }
    // Flow gates (engine extension, sph_abi.h "flow gates"): up to SPH_MAX_GATES oriented planar patches fixed in the
    // world; every substep from now on books, on the device, what crosses each of them (counts, fp64 sums of velocity and scalar values),
    // and with history > 0 stores the cumulative books every `stride` substeps in a ring.  An empty vector clears the table.  Gate() and
    // GateBox() build the records (GateBox: six rectangles with outward normals, -x +x -y +y -z +z).  SetGates does not synchronise;
    // GateBooks and GateHistory (rows oldest first, row k, gate i at rows[k * gates + i]) do.  Return false on error (LastError()).
    static SphGate Gate(int shape, const float center[3], const float u[3], const float v[3], bool unbounded = false) {
        SphGate g = SphGate();
        g.shape = shape; g.flags = unbounded ? SPH_GATE_UNBOUNDED : 0;
        for (int a = 0; a < 3; ++a) { g.center[a] = center[a]; g.u[a] = u[a]; g.v[a] = v[a]; }
        return g;
    }
    static std::vector<SphGate> GateBox(const float center[3], const float half[3]) {
        std::vector<SphGate> out;
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, d = (a + 2) % 3;
            for (int side = 0; side < 2; ++side) {
                const float sign = side ? 1.0f : -1.0f;
                float ce[3] = {center[0], center[1], center[2]}, u[3] = {0.0f, 0.0f, 0.0f}, v[3] = {0.0f, 0.0f, 0.0f};
                ce[a] += sign * half[a];
                u[b] = half[b]; v[d] = sign * half[d];                       // cross(e_b, e_d) = e_a
                out.push_back(Gate(SPH_GATE_RECT, ce, u, v));
            }
        }
        return out;
    }
    bool SetGates(const std::vector<SphGate>& gates, uint32_t history = 0, uint32_t stride = 1) {
        return !Check(sph_gates_set(engine, gates.empty() ? nullptr : gates.data(), int(gates.size()), history, stride), "sph_gates_set");
    }
    bool GetGates(std::vector<SphGate>& out) {
        int count = 0;
        out.resize(SPH_MAX_GATES);
        if (Check(sph_gates_get(engine, out.data(), SPH_MAX_GATES, &count, nullptr, nullptr), "sph_gates_get")) return false;
        out.resize(size_t(count));
        return true;
    }
    bool GateBooks(std::vector<SphGateBooks>& books, double& time, uint64_t& substeps, bool reset = false) {
        int count = 0;
        if (Check(sph_gates_get(engine, nullptr, 0, &count, nullptr, nullptr), "sph_gates_get")) return false;
        books.assign(size_t(count), SphGateBooks());
        return !Check(sph_gates_books(engine, books.empty() ? nullptr : books.data(), &time, &substeps, reset ? 1 : 0), "sph_gates_books");
    }
    bool GateHistory(std::vector<SphGateBooks>& rows, std::vector<double>& times, uint32_t& stored, uint64_t& firstRow) {
        int count = 0;
        uint32_t history = 0;
        if (Check(sph_gates_get(engine, nullptr, 0, &count, &history, nullptr), "sph_gates_get")) return false;
        rows.assign(size_t(history) * size_t(count), SphGateBooks());
        times.assign(history, 0.0);
        if (Check(sph_gates_history(engine, &firstRow, &stored, rows.empty() ? nullptr : rows.data(), times.empty() ? nullptr : times.data()), "sph_gates_history")) return false;
        rows.resize(size_t(stored) * size_t(count));
        times.resize(stored);
        return true;
    }
    // Field monitors (engine extension, sph_abi.h "field monitors"): up to SPH_MAX_MONITORS fixed sets of points, explicit
    // or a lattice origin + i * spacing (x fastest); every `every`-th substep from now on adds, on the device and inside the substep, the
    // SphSample of each point to the point's running fp64 sums (SphMonitorRow), and with history > 0 keeps the raw samples of the first
    // ringPoints points in a ring.  MonitorConfig() gives the defaults.  A set call restarts its slot; ResetMonitor zeroes rows, counters and
    // ring and keeps the buffers (averaging after a spin-up).  SetMonitor* and ResetMonitor do not synchronise; MonitorInfo, DownloadMonitor,
    // MonitorHistory (rows oldest first, row k, point p at samples[k * ringPoints + p]) and MonitorField do.  MonitorField derives the field
    // on the host from the downloaded rows with sph_monitor_field_host (the device's bytes); MonitorFieldDevice writes M floats into device
    // memory on the engine's stream.  Return false on error (LastError()).
    static SphMonitorConfig MonitorConfig() {
        SphMonitorConfig c;
        sph_monitor_config_default(&c);
        return c;
    }
    bool SetMonitor(int slot, const std::vector<MATH::Vec4>& points, const SphMonitorConfig& config) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        return !Check(sph_monitor_set(engine, slot, points.empty() ? nullptr : &points[0].x, points.size(), &config), "sph_monitor_set");
    }
    bool SetMonitorLattice(int slot, const MATH::Vec3& origin, const MATH::Vec3& spacing, const int dims[3], const SphMonitorConfig& config) {
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return false;
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        return !Check(sph_monitor_set_lattice(engine, slot, o, s, dims, &config), "sph_monitor_set_lattice");
    }
    bool MonitorInfo(int slot, SphMonitorInfo& out) { return !Check(sph_monitor_info(engine, slot, &out), "sph_monitor_info"); }
    bool DownloadMonitor(int slot, std::vector<SphMonitorRow>& rows) {
        SphMonitorInfo info;
        if (!MonitorInfo(slot, info)) return false;
        rows.assign(size_t(info.points), SphMonitorRow());
        return !Check(sph_monitor_download(engine, slot, rows.empty() ? nullptr : rows.data(), rows.size()), "sph_monitor_download");
    }
    bool MonitorHistory(int slot, std::vector<SphSample>& samples, std::vector<double>& times, uint32_t& stored, uint64_t& firstRow) {
        SphMonitorInfo info;
        if (!MonitorInfo(slot, info)) return false;
        samples.assign(size_t(info.config.history) * size_t(info.config.ringPoints), SphSample());
        times.assign(info.config.history, 0.0);
        if (Check(sph_monitor_history(engine, slot, &firstRow, &stored, samples.empty() ? nullptr : samples.data(), times.empty() ? nullptr : times.data(),
                                      info.config.history), "sph_monitor_history")) return false;
        samples.resize(size_t(stored) * size_t(info.config.ringPoints));
        times.resize(stored);
        return true;
    }
    bool MonitorField(int slot, int field, std::vector<float>& out) {
        std::vector<SphMonitorRow> rows;
        if (!DownloadMonitor(slot, rows)) return false;
        out.assign(rows.size(), 0.0f);
        return !Check(sph_monitor_field_host(rows.empty() ? nullptr : rows.data(), rows.size(), field, out.empty() ? nullptr : out.data()), "sph_monitor_field_host");
    }
    bool MonitorFieldDevice(int slot, int field, float* devOut) { return !Check(sph_monitor_field(engine, slot, field, devOut), "sph_monitor_field"); }
    bool ResetMonitor(int slot) { return !Check(sph_monitor_reset(engine, slot), "sph_monitor_reset"); }
    bool ClearMonitor(int slot = -1) { return !Check(sph_monitor_clear(engine, slot), "sph_monitor_clear"); }
    // Kinematic solid obstacles (engine extension, sph_abi.h "obstacles"): up to SPH_MAX_OBSTACLES bodies whose
    // motion the caller prescribes; every substep keeps the fluid out of them, advances their poses on the device and sums, per body,
    // the impulse (Jx, Jy, Jz, Lx, Ly, Lz) the fluid gave it.  An empty vector drops the set.  SetObstacleMotion keeps the device's pose
    // and does not synchronise; GetObstacles and ObstacleImpulses do.  Return false on error (LastError()).
    bool SetObstacles(const std::vector<SphObstacle>& obs) {
        return !Check(sph_obstacles_set(engine, obs.empty() ? nullptr : obs.data(), int(obs.size())), "sph_obstacles_set");
    }
    bool SetObstacleMotion(int index, const MATH::Vec3& vel, const MATH::Vec3& omega) {
        const float v[3] = {vel.x, vel.y, vel.z}, w[3] = {omega.x, omega.y, omega.z};
        return !Check(sph_obstacles_set_motion(engine, index, v, w), "sph_obstacles_set_motion");
    }
    bool GetObstacles(std::vector<SphObstacle>& out) {
        out.resize(SPH_MAX_OBSTACLES);
        int k = 0;
        if (Check(sph_obstacles_get(engine, out.data(), int(out.size()), &k), "sph_obstacles_get")) return false;
        out.resize(size_t(k));
        return true;
    }
    // impulses6: 6 doubles per body; time: simulated seconds and substeps they were summed over; reset zeroes them after the read.
    bool ObstacleImpulses(std::vector<double>& impulses6, double& time, uint64_t& substeps, bool reset = false) {
        impulses6.assign(6 * SPH_MAX_OBSTACLES, 0.0);
        if (Check(sph_obstacles_impulses(engine, impulses6.data(), SPH_MAX_OBSTACLES, &time, &substeps, reset ? 1 : 0), "sph_obstacles_impulses")) return false;
        std::vector<SphObstacle> cur;
        if (!GetObstacles(cur)) return false;
        impulses6.resize(6 * cur.size());
        return true;
    }
    // Triangle-mesh obstacles through signed distance lattices (engine extension, sph_abi.h "signed distance lattices", DESIGN.md section
    // 3f).  CreateVolume copies a lattice of signed distances (negative inside, x fastest) from host memory; VolumeFromMesh builds one on
    // the device from a closed mesh (triangles counter-clockwise seen from outside), centred on `center`; half receives the box size
    // that covers the lattice.  BindObstacleVolume(index, id) gives body `index` (a box) the volume's shape (id < 0 unbinds; SetObstacles
    // clears every binding).  MeshDistance writes the signed distances of a caller's lattice into a DEVICE array.  Return false on error.
    bool CreateVolume(const std::vector<float>& values, const int dims[3], const MATH::Vec3& spacing, int& id) {
        const float s[3] = {spacing.x, spacing.y, spacing.z};
        if (values.size() != size_t(dims[0]) * size_t(dims[1]) * size_t(dims[2])) { lastError = "CreateVolume: dims do not match the values"; return false; }
        return !Check(sph_volume_create(engine, values.data(), dims, s, 0, &id), "sph_volume_create");
    }
    bool VolumeFromMesh(const std::vector<float>& vertices3, const std::vector<uint32_t>& triangles3, const MATH::Vec3& center, float spacing,
                        const int dims[3], int& id, MATH::Vec3& half) {
        const float c[3] = {center.x, center.y, center.z}, s[3] = {spacing, spacing, spacing};
        if (Check(sph_volume_from_mesh(engine, vertices3.data(), vertices3.size() / 3, triangles3.data(), triangles3.size() / 3, c, s, dims, &id),
                  "sph_volume_from_mesh")) return false;
        float h[3];
        if (Check(sph_volume_info(engine, id, nullptr, nullptr, h), "sph_volume_info")) return false;
        half = MATH::Vec3(h[0], h[1], h[2]);
        return true;
    }
    // Dynamic rigid bodies (engine extension, sph_abi.h "dynamic rigid bodies"): a body with a dynamics record moves
    // under the fluid's impulses, gravity and the container, on the device, inside the substep.  SetObstacleDynamics(index, nullptr)
    // makes the body kinematic again; SetObstacles clears every record.  VolumeMoments returns the ten moments of the solid a volume
    // describes (cell volume times the weighted sums of 1, x, y, z, xx, yy, zz, xy, xz, yz), for the mass properties of a mesh body.
    bool SetObstacleDynamics(int index, const SphObstacleDynamics* dyn) {
        return !Check(sph_obstacles_set_dynamics(engine, index, dyn), "sph_obstacles_set_dynamics");
    }
    bool GetObstacleDynamics(int index, SphObstacleDynamics& out, bool& dynamic) {
        int on = 0;
        if (Check(sph_obstacles_get_dynamics(engine, index, &out, &on), "sph_obstacles_get_dynamics")) return false;
        dynamic = on != 0;
        return true;
    }
    bool VolumeMoments(int id, double out[10]) { return !Check(sph_volume_moments(engine, id, out), "sph_volume_moments"); }
    bool DestroyVolume(int id) { return !Check(sph_volume_destroy(engine, id), "sph_volume_destroy"); }
    bool BindObstacleVolume(int index, int id) { return !Check(sph_obstacles_bind_volume(engine, index, id), "sph_obstacles_bind_volume"); }
    bool MeshDistance(const std::vector<float>& vertices3, const std::vector<uint32_t>& triangles3, const MATH::Vec3& origin, const MATH::Vec3& spacing,
                      const int dims[3], float* devOut) {
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {spacing.x, spacing.y, spacing.z};
        return !Check(sph_mesh_distance(engine, vertices3.data(), vertices3.size() / 3, triangles3.data(), triangles3.size() / 3, o, s, dims, devOut),
                      "sph_mesh_distance");
    }
    bool Download(std::vector<SPHParticle>& out) {
        out.resize(sph_num_particles(engine));
        return !Check(sph_download_particles(engine, reinterpret_cast<SphParticle*>(out.data()), out.size()), "sph_download_particles");
    }
    // ---- checkpoints (sph_abi.h "checkpoints"): SaveState pushes the members first, as a dispatch would; LoadState makes the engine what
    // the saved one was and refreshes every member this class mirrors (param_*, fountain*, river*, terrainHeights, particles, numParticles,
    // stencilCount, the grid).  A refused blob leaves engine and members as they were.  All three synchronise.  Return false on error.
    bool SaveState(std::vector<unsigned char>& blob) {
        if (PushMembers()) return false;
        size_t need = 0;
        if (Check(sph_state_size(engine, &need), "sph_state_size")) return false;
        blob.assign(need, 0);
        return !Check(sph_state_save(engine, blob.data(), blob.size(), &need), "sph_state_save");
    }
    bool LoadState(const void* blob, size_t bytes) {
        SphStateInfo info;
        if (Check(sph_state_peek(blob, bytes, &info), "sph_state_peek") || Check(sph_state_load(engine, blob, bytes), "sph_state_load")) return false;
        SphParams p;
        SphFountain f;
        SphRiver r;
        if (Check(sph_get_params(engine, &p), "sph_get_params") || Check(sph_get_fountain(engine, &f), "sph_get_fountain") ||
            Check(sph_get_river(engine, &r), "sph_get_river")) return false;
        FromParams(p);
        fountainMode = f.fountainMode != 0; fountainOffset = MATH::Vec3(f.fountainOffset[0], f.fountainOffset[1], f.fountainOffset[2]);
        fountainRadius = f.fountainRadius; fountainSpread = f.fountainSpread; fountainJetSpeedLive = f.fountainJetSpeedLive;
        fountainDrainLevel = f.fountainDrainLevel; fountainDrainPerSec = f.fountainDrainPerSec; fountainSeed = f.fountainSeed;
        riverMode = r.riverMode != 0; terrainW = r.terrainW; terrainH = r.terrainH;
        terrainWorldMinX = r.terrainWorldMinX; terrainWorldMinZ = r.terrainWorldMinZ; terrainWorldSizeX = r.terrainWorldSizeX; terrainWorldSizeZ = r.terrainWorldSizeZ;
        riverEmitterPos = MATH::Vec3(r.riverEmitterPos[0], r.riverEmitterPos[1], r.riverEmitterPos[2]);
        riverEmitterVel = MATH::Vec3(r.riverEmitterVel[0], r.riverEmitterVel[1], r.riverEmitterVel[2]);
        riverEmitterRadius = r.riverEmitterRadius; riverSinkY = r.riverSinkY; riverSinkZMax = r.riverSinkZMax;
        riverAmp = r.riverAmp; riverFreq = r.riverFreq; riverPhase = r.riverPhase;
        riverChannelWidth = r.riverChannelWidth; riverChannelDepth = r.riverChannelDepth; riverSlopeDrop = r.riverSlopeDrop;
        terrainHeights.resize(size_t(info.terrainCount));
        if (info.terrainCount) std::memcpy(terrainHeights.data(), static_cast<const unsigned char*>(blob) + info.terrainOffset, 4 * size_t(info.terrainCount));
        terrainDirty = false;
        stencilCount = int(info.stencilCount);
        numParticles = size_t(info.n);
        surface = SphSurface{};
        AfterSpawn();
        return true;
    }
    bool StateDigest(SphStateDigest& out, uint32_t sections = 0) {
        if (PushMembers()) return false;
        return !Check(sph_state_digest(engine, sections, &out), "sph_state_digest");
    }
    static bool PeekState(const void* blob, size_t bytes, SphStateInfo& out) { return sph_state_peek(blob, bytes, &out) == SPH_OK; }
    void Sync() { Check(sph_sync(engine), "sph_sync"); }
    const std::string& LastError() const { return lastError; }
    SphEngine* Handle() { return engine; }

    // ---- public data members, names and defaults of SPHFluid3D.h:62-124 ------------------
    float box = 7.0f;
    float cellSize = 0.0f;
    int gridSizeX = 1, gridSizeY = 1, gridSizeZ = 1;
    int numCells = 1;
    MATH::Vec3 gridMinV = MATH::Vec3(-7, -7, -7);
    std::vector<SPHParticle> particles;        // initial state only, never refreshed (as in the reference)
    size_t numParticles;
    size_t numFluids = 0;

    float param_h = 0.28f;
    float param_mass = 13.8f;
    float param_restDensity = 1000.0f;
    float param_gasConstant = 2000.0f;
    float param_viscosity = 3.5f;
    float param_gravityY = -980.0f;
    float param_gravityX = 0.0f;
    float param_gravityZ = 0.0f;
    float param_surfaceTension = 0.0728f;
    float param_timeStep = 0.001f;
    bool param_pause = false;
    bool param_useJitter = true;
    float param_jitterAmp = 0.20f;
    float param_foamGen = 1.0f;
    float param_foamVelRef = 8.0f;
    MATH::Vec3 param_boxCenter = MATH::Vec3(0, 0, 0);
    MATH::Vec3 param_boxHalf = MATH::Vec3(7, 7, 7);
    MATH::Vec3 param_boxEulerDeg = MATH::Vec3(0, 0, 0);
    int param_shapeType = 0;
    MATH::Vec3 param_shapeAux = MATH::Vec3(5.0f, 0.35f, 2.5f);
    int param_mixPattern = 0;
    int param_dyePattern = 0;
    float param_wallRestitution = 0.15f;
    float param_wallFriction = 0.02f;
    // inert counterpart of a member Scene0p touches (SPHFluid3D.h:72 `ssbo`: bound as binding 0 by the GL renderers,
    // Scene0p.cpp:1625,2627,3065,3142 -- 0 binds nothing)
    unsigned int ssbo = 0;
    // river / stream mode, SPHFluid3D.h:171-196 (step 5 of DispatchCompute, :511-516; Scene0p only ever writes
    // riverMode = false, Scene0p.cpp:1660).  After editing terrainHeights by hand set terrainDirty.
    bool riverMode = false;
    std::vector<float> terrainHeights;
    int terrainW = 64, terrainH = 64;
    float terrainWorldMinX = -7.0f, terrainWorldMinZ = -10.0f, terrainWorldSizeX = 14.0f, terrainWorldSizeZ = 20.0f;
    MATH::Vec3 riverEmitterPos = MATH::Vec3(0.0f, 3.0f, -9.0f);
    MATH::Vec3 riverEmitterVel = MATH::Vec3(0.0f, -0.5f, 4.0f);
    float riverEmitterRadius = 1.5f, riverSinkY = -8.5f, riverSinkZMax = 9.0f;
    float riverAmp = 2.0f, riverFreq = 0.25f, riverPhase = 0.0f, riverChannelWidth = 3.0f, riverChannelDepth = 3.5f, riverSlopeDrop = 0.3f;
    bool terrainDirty = false;                 // engine extension: terrainHeights changed since the last upload
    // fountain members, SPHFluid3D.h:161-168 (step 6 of DispatchCompute, :519)
    bool fountainMode = false;
    MATH::Vec3 fountainOffset = MATH::Vec3(0.0f, -5.0f, 0.0f);
    float fountainRadius = 1.0f;
    float fountainSpread = 0.25f;
    float fountainJetSpeedLive = 25.0f;
    float fountainDrainLevel = 1.0f;
    float fountainDrainPerSec = 2.0f;
    unsigned fountainSeed = 0;
    int grid_cap = 160;                        // engine extension (SPHFluid3D.cpp:370 hard-codes 160)
    uint32_t seed;                             // engine extension (the reference seeds from time(nullptr), :99)

private:
    SphEngine* engine = nullptr;
    void* stream = nullptr;
    std::string lastError;
    SphSurface surface{};                      // counts of the last ExtractSurface (DownloadSurface sizes its vectors from them)

    SphRiver ToRiver() const {
        return SphRiver{riverMode ? 1 : 0, terrainW, terrainH, terrainWorldMinX, terrainWorldMinZ, terrainWorldSizeX, terrainWorldSizeZ,
                        {riverEmitterPos.x, riverEmitterPos.y, riverEmitterPos.z}, {riverEmitterVel.x, riverEmitterVel.y, riverEmitterVel.z},
                        riverEmitterRadius, riverSinkY, riverSinkZMax, riverAmp, riverFreq, riverPhase, riverChannelWidth, riverChannelDepth,
                        riverSlopeDrop};
    }
    bool PushRiver() {                         // true on error
        const SphRiver r = ToRiver();
        const bool send = terrainDirty && terrainHeights.size() == size_t(terrainW) * size_t(terrainH);
        if (Check(sph_set_river(engine, &r, send ? terrainHeights.data() : nullptr), "sph_set_river")) return true;
        if (send) terrainDirty = false;
        return false;
    }
    bool PushMembers() {                       // what DispatchCompute sends ahead of a substep; true on error
        SphParams p = ToParams();
        if (Check(sph_set_params(engine, &p), "sph_set_params")) return true;
        SphFountain f{fountainMode ? 1 : 0, {fountainOffset.x, fountainOffset.y, fountainOffset.z}, fountainRadius, fountainSpread,
                      fountainJetSpeedLive, fountainDrainLevel, fountainDrainPerSec, fountainSeed};
        if (Check(sph_set_fountain(engine, &f), "sph_set_fountain")) return true;
        return PushRiver();
    }
    SphParams ToParams() const {
        SphParams p;
        sph_params_default(&p);
        p.param_h = param_h; p.param_mass = param_mass; p.param_restDensity = param_restDensity;
        p.param_gasConstant = param_gasConstant; p.param_viscosity = param_viscosity;
        p.param_gravityY = param_gravityY; p.param_gravityX = param_gravityX; p.param_gravityZ = param_gravityZ;
        p.param_surfaceTension = param_surfaceTension; p.param_timeStep = param_timeStep;
        p.param_pause = param_pause ? 1 : 0; p.param_useJitter = param_useJitter ? 1 : 0; p.param_jitterAmp = param_jitterAmp;
        p.param_foamGen = param_foamGen; p.param_foamVelRef = param_foamVelRef;
        const MATH::Vec3* v[4] = {&param_boxCenter, &param_boxHalf, &param_boxEulerDeg, &param_shapeAux};
        float* d[4] = {p.param_boxCenter, p.param_boxHalf, p.param_boxEulerDeg, p.param_shapeAux};
        for (int i = 0; i < 4; ++i) { d[i][0] = v[i]->x; d[i][1] = v[i]->y; d[i][2] = v[i]->z; }
        p.param_shapeType = param_shapeType; p.param_mixPattern = param_mixPattern; p.param_dyePattern = param_dyePattern;
        p.param_wallRestitution = param_wallRestitution; p.param_wallFriction = param_wallFriction;
        p.grid_cap = grid_cap;
        return p;
    }
    void FromParams(const SphParams& p) {
        param_h = p.param_h; param_mass = p.param_mass; param_restDensity = p.param_restDensity;
        param_gasConstant = p.param_gasConstant; param_viscosity = p.param_viscosity;
        param_gravityY = p.param_gravityY; param_gravityX = p.param_gravityX; param_gravityZ = p.param_gravityZ;
        param_surfaceTension = p.param_surfaceTension; param_timeStep = p.param_timeStep;
        param_pause = p.param_pause != 0; param_useJitter = p.param_useJitter != 0; param_jitterAmp = p.param_jitterAmp;
        param_foamGen = p.param_foamGen; param_foamVelRef = p.param_foamVelRef;
        param_boxCenter = MATH::Vec3(p.param_boxCenter[0], p.param_boxCenter[1], p.param_boxCenter[2]);
        param_boxHalf = MATH::Vec3(p.param_boxHalf[0], p.param_boxHalf[1], p.param_boxHalf[2]);
        param_boxEulerDeg = MATH::Vec3(p.param_boxEulerDeg[0], p.param_boxEulerDeg[1], p.param_boxEulerDeg[2]);
        param_shapeType = p.param_shapeType;
        param_shapeAux = MATH::Vec3(p.param_shapeAux[0], p.param_shapeAux[1], p.param_shapeAux[2]);
        param_mixPattern = p.param_mixPattern; param_dyePattern = p.param_dyePattern;
        param_wallRestitution = p.param_wallRestitution; param_wallFriction = p.param_wallFriction;
        grid_cap = p.grid_cap;
    }
    void SetGrid(const SphGridInfo& g) {
        gridSizeX = g.dims[0]; gridSizeY = g.dims[1]; gridSizeZ = g.dims[2]; numCells = g.numCells;
        gridMinV = MATH::Vec3(g.gridMin[0], g.gridMin[1], g.gridMin[2]); cellSize = g.cellSize;
    }
    void RefreshGrid() {
        SphGridInfo g;
        if (!Check(sph_grid_info(engine, &g), "sph_grid_info")) SetGrid(g);
    }
    void AfterSpawn() {
        SphParams p;
        if (!Check(sph_get_params(engine, &p), "sph_get_params")) param_mass = p.param_mass;   // SPHFluid3D.cpp:92
        particles.resize(sph_num_particles(engine));
        Check(sph_initial_particles(engine, reinterpret_cast<SphParticle*>(particles.data()), particles.size()), "sph_initial_particles");
        numFluids = 0;
        for (const auto& q : particles) if (q.isGhost == 0) ++numFluids;                       // SPHFluid3D.cpp:338-339
        box = param_boxHalf.x > param_boxHalf.y ? (param_boxHalf.x > param_boxHalf.z ? param_boxHalf.x : param_boxHalf.z)
                                                : (param_boxHalf.y > param_boxHalf.z ? param_boxHalf.y : param_boxHalf.z);
        RefreshGrid();
        std::printf("Fluid particles: %zu\n", particles.size());
    }
    void Create() {
        SphParams p = ToParams();
        if (Check(sph_create(&engine, numParticles, &p, seed, stream), "sph_create")) return;
        AfterSpawn();
    }
    bool Check(int rc, const char* what) {     // logs like Debug::FatalError (which only logs, Debug.cpp:54)
        if (rc == SPH_OK) return false;
        lastError = std::string(what) + ": " + sph_last_error();
        std::fprintf(stderr, "SPHFluidGPU(HIP) %s\n", lastError.c_str());
        return true;
    }
};
