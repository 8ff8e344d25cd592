/*
 * sph_abi.h -- C-ABI of the MI355X-native SPH substep engine (libsph_hip.so).
 *
 * The reference has no plugin/FFI layer: its boundary is the concrete C++ class
 * SPHFluidGPU (ComponentFramework/SPHFluid3D.h:26-210) that Scene0p holds by raw
 * pointer (Scene0p.h:396).  Each entry point below names the reference member it
 * replaces.  Plain pointers and sizes only; no torch / STL types cross this line.
 * The header-only C++ shim include/SPHFluidGPU_hip.hpp re-creates the class surface
 * (same member names) on top of these calls; INTEGRATION.md shows the swap.
 *
 * Conventions
 *  - every function returns 0 on success, a negative SPH_ERR_* otherwise, and
 *    leaves a message for sph_last_error() (thread-local);
 *  - calls enqueue work on the engine's HIP stream and return without waiting;
 *    sph_download_particles() and sph_sync() synchronise;
 *  - one host thread per engine (as the reference: everything runs on the GL thread,
 *    SceneManager.cpp:69-93);
 *  - there is NO CPU fallback: without a HIP device every compute call fails with
 *    SPH_ERR_HIP.
 */
#ifndef SPH_ABI_H
#define SPH_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_ABI_VERSION 4   /* 4: the PLAN of a sized exchange (SphSlabIntent) compared between neighbours before any record moves: sph_slab_step_finish_local compares the
                               neighbour engines' plans, the RCCL transport sends them across each link first (sph_slab_set_verify), waits with a deadline (SPH_ERR_TIMEOUT,
                               sph_slab_set_deadline, sph_sync_deadline); flag 32; sph_slab_plan / _plans_agree, sph_comm_selftest_faces; SPH_OPT_NEIGHBOR_KERNEL 4 retired */
/* (still 4, additions only: SphSample, SPH_FIELD_*, sph_sample_points / sph_sample_points_device / sph_sample_lattice -- field sampling) */
/* (still 4, additions only: SphSurfaceVertex, SphSurface, sph_extract_surface / sph_extract_surface_volume / sph_surface_download -- iso-surface meshes) */
/* (still 4, additions only: SphStatistics, SphStatExtremum, SphHistogramSpec, SPH_STAT_*, sph_statistics / sph_statistics_device -- state statistics) */
/* (still 4, additions only: SphTracer, SPH_TRACER_*, sph_tracers_set / _set_device / _count / _info / _download / _device / _history -- passive tracers) */
/* (still 4, additions only: SPH_MAX_SCALAR_CHANNELS, SPH_SCALAR_*, sph_scalars_set / _set_device / _set_coefficients / _channels / _download / _device /
    _paint / _info / _moments / _sample_points / _sample_points_device / _sample_lattice / _step_host, SphScalarMoments, SPH_OPT_SCALAR_SWEEP -- diffusing scalar fields carried by the particles) */
/* (still 4, additions only: SphObstacle, SPH_OBSTACLE_*, SPH_MAX_OBSTACLES, sph_obstacle_default, sph_obstacles_set / _set_motion / _get / _impulses /
    _apply_host / _advance_host -- kinematic solid obstacles) */
/* (still 4, additions only: SphVolumeHost, SPH_MAX_VOLUMES, SPH_OPT_MESH_SPLIT, sph_volume_create / _destroy / _info / _sample_host / _from_mesh,
    sph_obstacles_bind_volume / _volume / _apply_host_volumes, sph_mesh_distance / _host -- triangle-mesh obstacles through signed distance lattices) */
/* (still 4, additions only: SphObstacleDynamics, SPH_DYNAMICS_CONFINED, sph_obstacle_dynamics_default, sph_obstacles_set_dynamics / _get_dynamics /
    _step_host, sph_volume_moments / _host -- dynamic rigid bodies) */
/* (still 4, additions only: SphScalarSource, SPH_MAX_SCALAR_SOURCES, SPH_SOURCE_*, sph_scalar_source_default, sph_scalars_set_buoyancy / _get_buoyancy /
    _set_sources / _get_sources / _injected / _couple_host -- active scalars: buoyancy and continuous sources) */
/* (still 4, additions only: SphGate, SphGateBooks, SPH_MAX_GATES, SPH_MAX_GATE_HISTORY, SPH_GATE_*, sph_gates_set / _get / _books / _history / _step_host -- flow gates) */
/* (still 4, additions only: SphMonitorConfig, SphMonitorRow, SphMonitorInfo, SPH_MAX_MONITORS, SPH_MAX_MONITOR_POINTS, SPH_MAX_MONITOR_HISTORY, SPH_MONITOR_*,
    sph_monitor_config_default / _set / _set_device / _set_lattice / _info / _download / _device / _history / _field / _reset / _clear / _accumulate_host /
    _field_host / _schedule_host -- field monitors: probes and lattices averaged inside the substep) */
/* (still 4, additions only: SphDiffuse, SphDiffuseConfig, SphDiffuseInfo, SPH_DIFFUSE_*, sph_diffuse_default / _set / _get / _info / _download / _device /
    _seed / _step_host, SPH_OPT_DIFFUSE_TIMED -- spray, foam and bubbles: secondary particles spawned by the fluid) */
/* (still 4, additions only: SphDiffuseCrest, SphDiffuseCrestInfo, sph_diffuse_crest_default / _crest_info, sph_diffuse_set_crest / _get_crest,
 * sph_diffuse_step_host_crest -- spray and foam born at wave crests) */
/* (still 4, additions only: SphNeighborInfo, SPH_NEIGHBORS_*, sph_neighbors_build / _query / _info / _device / _export / _download / _host, SPH_OPT_NEIGHBORS_FILL -- neighbour lists) */
/* (still 4, additions only: SphComponent, SphComponentInfo, SPH_COMPONENTS_FLUID_ONLY, SPH_COMPONENT_NONFINITE, sph_components_build / _info / _device / _download / _host, SPH_OPT_COMPONENTS_VARIANT -- connected bodies of fluid) */
/* (still 4, additions only: SphKnnInfo, SPH_KNN_SELF, SPH_KNN_FLUID_ONLY, SPH_KNN_MAX_K, sph_knn_build / _query / _info / _device / _download / _host, SPH_OPT_KNN_VARIANT -- k nearest neighbours) */
/* (still 4, additions only: SphRayHit, SphRaysInfo, SPH_RAYS_FLUID_ONLY, SPH_RAYS_ANY_HIT, sph_rays_cast / _cast_device / _info / _device / _download / _host / _walk_host, SPH_OPT_RAYS_VARIANT -- ray casts against the particles) */
/* (still 4, additions only: SphRaySpan, SphRaySpansInfo, sph_rays_span / _span_device / _span_info / _span_rows / _span_download / _span_host / _span_walk_host, SPH_OPT_RAY_SPANS_VARIANT -- ray spans: what each ray crosses in all) */
/* (still 4, additions only: SphAniso, SphAnisoConfig, SphAnisoInfo, SPH_ANISO_FLUID_ONLY, SPH_ANISO_VALID / _SPARSE / _CLAMPED, sph_aniso_default / _build / _info / _device / _download / _lattice / _surface / _host / _lattice_host -- anisotropic kernels) */
/* (still 4, additions only: SphShell, SphShellConfig, SphShellInfo, SPH_SHELL_FLUID_ONLY, SPH_SHELL_MEMBER, SPH_SHELL_ISOLATED, sph_shell_default / _build / _query / _info / _device / _download / _host, SPH_OPT_SHELL_TIMED -- free-surface particles) */
/* (still 4, additions only: SphStateInfo, SphStateDigest, SPH_STATE_*, sph_state_size / _save / _load / _peek / _digest / _checksum_host -- checkpoints) */
/* (still 4, additions only: SphAggregateConfig, SphAggregateInfo, SPH_AGGREGATE_*, sph_aggregate_default / _particles / _query / _staged / _host, SPH_OPT_AGGREGATE_VARIANT -- fused neighbourhood reductions of caller tensors) */
/* (still 4, additions only: sph_aggregate_adjoint_particles / _query / _staged / _host, sph_aggregate_arg_particles / _query / _host, sph_aggregate_route_particles / _query / _host -- the adjoint of the neighbourhood sums, extrema with their winners, routing through them) */
/* (still 4, additions only: SPH_SLAB_FLAG_* -- names of the six bits of the z-slab exchange's flag word, values as before) */
/* (still 4, additions only: SphBasisConfig, SPH_BASIS_GRID, sph_aggregate_basis_default / _particles / _query / _staged / _host, sph_aggregate_basis_adjoint_particles / _query / _staged / _host -- filter-grid basis sums: continuous convolutions without an edge list) */
/* (still 4, additions only: sph_aggregate_posgrad_particles / _query / _staged / _host -- position gradients of the neighbourhood sums) */
/* (still 4, additions only: sph_aggregate_basis_posgrad_particles / _query / _staged / _host -- position gradients of the basis sums) */
/* (3: compact halo faces (40-byte halo copies, count-sized messages), jumps of up to 3 cell layers followed, sph_slab_clear_flags / _message_bytes / _step_times / _face_bytes, flag 16 no longer an error, SPH_OPT_NEIGHBOR_KERNEL 4) */
/* (2: sph_slab_step_*, header validation of received halo messages, SPH_OPT_NEIGHBOR_KERNEL 3 (default), records on demand by default) */

enum {
    SPH_OK = 0,
    SPH_ERR_ARG = -1,      /* bad argument / null handle                    */
    SPH_ERR_HIP = -2,      /* HIP runtime error (message has hipGetErrorString) */
    SPH_ERR_STATE = -3,    /* call not valid in the engine's current state   */
    SPH_ERR_CAPACITY = -4, /* a fixed-capacity buffer (ghosts, migrants) overflowed */
    SPH_ERR_TIMEOUT = -5   /* a wait for a neighbour rank ran into its deadline (sph_slab_set_deadline): device work of this rank is still queued behind a
                              transfer that will never complete; print sph_last_error() and end the process */
};

/* 80-byte particle record: struct SPHParticle, SPHFluid3D.h:12-24 (std430 twin:
 * shaders/SPHFluid.comp:5-17).  Index i is the same particle forever (renderers
 * index by gl_InstanceID, Scene0p.cpp:1625-1637): the engine never permutes this
 * array, whatever it sorts internally. */
typedef struct SphParticle {
    float pos[4];
    float vel[4];
    float acc[4];
    float density;
    float pressure;
    float padA;      /* foam factor, SPHFluid.comp:209-217          */
    float padB;      /* dye, SPHFluid3D.cpp:316-329                 */
    int32_t isGhost;
    int32_t isActive;
    int32_t padC;    /* colour group, SPHFluid3D.cpp:307-311        */
    int32_t pad0;
} SphParticle;

/* The public param_* members of SPHFluidGPU, SPHFluid3D.h:94-124, field for field.
 * Sampled at every sph_dispatch(), like the per-dispatch uniform uploads at
 * SPHFluid3D.cpp:458-506, so edits take effect on the next substep. */
typedef struct SphParams {
    float param_h;                 /* :94  */
    float param_mass;              /* :95  (overwritten by spawn: rho0*(0.85h)^3, SPHFluid3D.cpp:92) */
    float param_restDensity;       /* :96  */
    float param_gasConstant;       /* :97  */
    float param_viscosity;         /* :98  */
    float param_gravityY;          /* :99  */
    float param_gravityX;          /* :100 */
    float param_gravityZ;          /* :101 */
    float param_surfaceTension;    /* :102 */
    float param_timeStep;          /* :103 */
    int32_t param_pause;           /* :104 (bool) */
    int32_t param_useJitter;       /* :106 (bool) */
    float param_jitterAmp;         /* :107 */
    float param_foamGen;           /* :109 */
    float param_foamVelRef;        /* :110 */
    float param_boxCenter[3];      /* :112 */
    float param_boxHalf[3];        /* :113 */
    float param_boxEulerDeg[3];    /* :116 */
    int32_t param_shapeType;       /* :117 */
    float param_shapeAux[3];       /* :119 */
    int32_t param_mixPattern;      /* :121 */
    int32_t param_dyePattern;      /* :122 */
    float param_wallRestitution;   /* :123 */
    float param_wallFriction;      /* :124 */
    /* engine extension, no reference member: per-axis cell-count cap of
     * ComputeGridExtents (hard-coded 160 at SPHFluid3D.cpp:370). */
    int32_t grid_cap;
} SphParams;

typedef struct SphGridInfo {       /* gridSizeX/Y/Z, numCells, gridMinV, cellSize: SPHFluid3D.h:63-66 */
    int32_t dims[3];
    int32_t numCells;
    float gridMin[3];
    float cellSize;
} SphGridInfo;

typedef struct SphFountain {       /* public fountain* members of SPHFluidGPU, SPHFluid3D.h:161-168 (same names) */
    int32_t fountainMode;          /* bool fountainMode = false */
    float fountainOffset[3];       /* nozzle, container-relative (0,-5,0) */
    float fountainRadius;          /* 1.0 */
    float fountainSpread;          /* 0.25 */
    float fountainJetSpeedLive;    /* 25.0, written per frame by the scene */
    float fountainDrainLevel;      /* 1.0 */
    float fountainDrainPerSec;     /* 2.0 */
    uint32_t fountainSeed;         /* advances by one per dispatch (SPHFluid3D.cpp:541) */
} SphFountain;

typedef struct SphRiver {          /* public river / terrain members of SPHFluidGPU, SPHFluid3D.h:171-196 (same names, same initialisers) */
    int32_t riverMode;             /* bool riverMode = false */
    int32_t terrainW, terrainH;    /* 64, 64: heightfield samples; the heights themselves travel beside this struct */
    float terrainWorldMinX, terrainWorldMinZ, terrainWorldSizeX, terrainWorldSizeZ;   /* -7, -10, 14, 20 */
    float riverEmitterPos[3];      /* (0, 3, -9) */
    float riverEmitterVel[3];      /* (0, -0.5, 4) */
    float riverEmitterRadius;      /* 1.5 */
    float riverSinkY, riverSinkZMax;   /* -8.5, 9 */
    float riverAmp, riverFreq, riverPhase, riverChannelWidth, riverChannelDepth, riverSlopeDrop;   /* 2, 0.25, 0, 3, 3.5, 0.3 */
} SphRiver;

typedef struct SphEngine SphEngine; /* opaque; owns every device buffer (as SPHFluidGPU owns its GL buffers, SPHFluid3D.cpp:61-83) */

/* ---- engine options (sph_set_option) ------------------------------------------- */
enum {
    SPH_OPT_NEIGHBOR_KERNEL = 1, /* SPH pass: 3 = k_sph_walk (default: one target per lane, LDS-staged candidate rows, neighbour lists walked per lane over 32-byte records), 2 = k_sph_list (round 2's form of the same plan), 1 = k_sph_slow (one target per thread, plain sweeps over global memory); same bits. 0 (round 1's tile pass) and 4 (round 4's k_sph_tile: measured slower everywhere, profiles/r04_tile_pass_experiment.txt) were retired and are refused */
    SPH_OPT_GRID_BUILD = 2,      /* 0 = counting sort (default), 1 = atomicExch linked list as BuildGrid.comp (A/B only; neighbour order then arbitrary) */
    SPH_OPT_AOS_MODE = 3,        /* 1 = lazy (default): the substep keeps its state in the engine's own arrays and the 80-byte records are brought up to date by sph_device_particles() / sph_download_particles() / sph_pack_render_buffer(), i.e. once per rendered frame instead of once per substep (the scattered 52-byte update of every record costs about 13 % of the SPH pass); 0 = eager: the SPH pass also updates the records, they are current after every dispatch. Same values either way. */
    SPH_OPT_GRAPH = 5,           /* 1 = sph_dispatch_n replays a hipGraph once the same call (same members, options, substep count) has been seen twice; default 0 */
    SPH_OPT_MESH_SPLIT = 7,      /* sph_mesh_distance: 0 = the engine chooses into how many ranges the triangles are split (default), 1..64 = that many (capped at one per 256 triangles); same bits */
    SPH_OPT_SCALAR_SWEEP = 8,    /* scalar channels (sph_scalars_*): 0 = the sweep walks global memory (default, the bit-level yardstick), 1 = a block of 256 consecutive slots stages its candidate rows in LDS first; same bits */
    SPH_OPT_DIFFUSE_TIMED = 9,   /* diffuse particles (sph_diffuse_*), measurements only: which launches of a substep the SPH_OPT_TIMING bracket covers -- 0 = all of them (default), 1 = the advance kernel, 2 = the spawn side (count, scans, compaction, emit, tick); the launches themselves are the same */
    SPH_OPT_NEIGHBORS_FILL = 10, /* neighbour lists (sph_neighbors_*), an A/B of the fill kernel: 0 = every lane writes the entries of its own row (default), 1 = a wave writes one row at a time with consecutive lanes; the same bits */
    SPH_OPT_COMPONENTS_VARIANT = 11, /* connected components (sph_components_*), A/Bs for measurements: bit 0 = the hook walks every candidate, not only those in front of the target's slot; bit 1 = the table kernel issues its atomics per lane, not once per wave and label; default 0; the same bits */
    SPH_OPT_KNN_VARIANT = 12,    /* k nearest neighbours (sph_knn_*), an A/B for measurements: 0 = one target per lane keeps its k best keys in LDS (default), 1 = k selection passes over the candidates without any storage (slow); the same bits */
    SPH_OPT_RAYS_VARIANT = 13,   /* ray casts (sph_rays_*), an A/B for measurements: 0 = the rays are cast in the caller's order (default), 1 = in the order of the grid cell they enter first (a counting sort of the rays in front of the walk: faster for incoherent rays, slower for sheets and fans); the same bits */
    SPH_OPT_SHELL_TIMED = 14,    /* free-surface particles (sph_shell_*), measurements only: which launches of a build the SPH_OPT_TIMING bracket covers -- 0 = all of them (default), 1 = pass 1 (ids and the gather), 2 = pass 2 (the crest kernel), 3 = the two scans and compactions; the launches themselves are the same */
    SPH_OPT_RAY_SPANS_VARIANT = 15, /* ray spans (sph_rays_span*), an A/B for measurements: 0 = the layer walk (default: after the first cell only the new 3 x 3 layer of the block is tested), 1 = the block walk (every step tests the whole block and drops what the previous cell's block held); the same bits.  SPH_OPT_RAYS_VARIANT orders the rays of spans as it does those of casts */
    SPH_OPT_AGGREGATE_VARIANT = 16, /* neighbourhood reductions (sph_aggregate_*), A/Bs for measurements: bit 0 = the payload is gathered by particle id straight from the caller's array (no staging into slot order); bits 1-2 = the channels per pass of the walk: 0 the default (the smallest of 4, 8, 16 that holds the channels), 1 = 4, 2 = 8, 3 = 16; bit 3 = 4-byte payload loads also where 16-byte loads apply; default 0; the same bits */
    SPH_OPT_GRAPH_LAUNCHES = 6,  /* read-only: number of graph replays so far */
    SPH_OPT_TIMING = 4,          /* hipEvents around kernels for sph_kernel_times(): 1 = every kernel, 2 = only the SPH pass */
    /* test / tuning hooks */
    SPH_OPT_DEBUG = 100          /* test hooks of k_sph_walk / k_sph_list -- bit 0: treat every neighbour list as overflowed, bit 1: treat every target as
                                    outside the list's slack (sweep-3 fallback), bit 2: treat every window as overflowed (whole wave falls
                                    back), bit 3: count fallbacks / list entries / staged candidates for sph_debug_counters
                                    (bit 8 is used internally by the z-slab face launch) */
};

/* ---- host-only helpers (no device needed) --------------------------------------- */
int sph_abi_version(void);
/* Defaults of SPHFluid3D.h:94-124 (+ grid_cap = 160). */
int sph_params_default(SphParams* out);
/* MakeRotationMat3XYZ, SPHFluid3D.cpp:13-30: column-major world_from_box. */
int sph_rotation_mat3(const float eulerDeg[3], float outM[9]);
/* SPHFluidGPU::EffectiveHalf(), SPHFluid3D.h:127-158. */
int sph_effective_half(const SphParams* params, float outHalf[3]);
/* SPHFluidGPU::ComputeGridExtents(), SPHFluid3D.cpp:354-376. */
int sph_compute_grid_extents(const SphParams* params, SphGridInfo* out);
/* SPHFluidGPU::InitializeParticles() standard-fill branch, SPHFluid3D.cpp:85-102,159-332,
 * with an explicit seed (the reference seeds from time(nullptr), :99).  Writes at most
 * nRequested records, returns the count produced through *nOut and param_mass (:92)
 * through *massOut. */
int sph_spawn_particles(const SphParams* params, size_t nRequested, uint32_t seed,
                        SphParticle* out, size_t* nOut, float* massOut);
const char* sph_last_error(void);

/* ---- lifetime ------------------------------------------------------------------- */
/* SPHFluidGPU::SPHFluidGPU(size_t), SPHFluid3D.cpp:32-59: spawn + allocate + upload.
 * `stream` is a hipStream_t (or NULL for an engine-owned stream). */
int sph_create(SphEngine** out, size_t nRequested, const SphParams* params, uint32_t seed, void* stream);
/* Same, but with caller-provided initial records instead of the spawn (bench / tests). */
int sph_create_from_particles(SphEngine** out, const SphParticle* particles, size_t n,
                              const SphParams* params, void* stream);
/* SPHFluidGPU::~SPHFluidGPU(), SPHFluid3D.cpp:61-83. */
int sph_destroy(SphEngine* e);
/* SPHFluidGPU::ResetSimulation(), SPHFluid3D.cpp:713-731: respawn with numParticles
 * requested (Scene0p.cpp:1403-1408 writes numParticles before the reset). Invalidates
 * the pointer returned by sph_device_particles(). */
int sph_reset(SphEngine* e, size_t nRequested, uint32_t seed);

/* ---- parameters ----------------------------------------------------------------- */
int sph_set_params(SphEngine* e, const SphParams* params);
int sph_get_params(const SphEngine* e, SphParams* out);
int sph_set_option(SphEngine* e, int option, int value);
int sph_get_option(const SphEngine* e, int option, int* value);

/* ---- the hot path ---------------------------------------------------------------- */
/* SPHFluidGPU::DispatchCompute(float overrideDt = -1), SPHFluid3D.cpp:431-522:
 * ClearGrid -> BuildGrid -> SPHFluid -> OBBConstraints. No-op when param_pause. */
int sph_dispatch(SphEngine* e, float overrideDt);
/* n back-to-back substeps (the reel-export loop, Scene0p.cpp:3720-3739). */
int sph_dispatch_n(SphEngine* e, float overrideDt, int nSubsteps);
/* SPHFluidGPU::ApplyWaveImpulse, SPHFluid3D.cpp:604-623 + shaders/WaveImpulse.comp. */
int sph_apply_wave_impulse(SphEngine* e, float amplitude, float wavelength, float phase,
                           const float dir[3], float yMin, float yMax);

/* SPHFluidGPU::ApplyVortexImpulse, SPHFluid3D.cpp:627-646 + shaders/VortexImpulse.comp (kicks pre-multiplied by dt). */
int sph_apply_vortex_impulse(SphEngine* e, float tangentKick, float inwardKick);
/* SPHFluidGPU::ApplyAttractorImpulse, SPHFluid3D.cpp:650-664 + shaders/AttractorImpulse.comp. */
int sph_apply_attractor_impulse(SphEngine* e, const float point[3], float pullKick, float radius);
/* SPHFluidGPU::SetStencilTargets, SPHFluid3D.cpp:684-693: `count` points of 4 floats (w unused). */
int sph_set_stencil_targets(SphEngine* e, const float* points4, size_t count);
/* SPHFluidGPU::ApplyStencilAttract, SPHFluid3D.cpp:695-710 + shaders/StencilAttract.comp (target = points[i % count]). */
int sph_apply_stencil_attract(SphEngine* e, float pullKick, float dampKick);
/* SPHFluidGPU::ApplyCurlFlow, SPHFluid3D.cpp:668-681 + shaders/CurlFlow.comp. */
int sph_apply_curl_flow(SphEngine* e, float kick, float scale, float time);

/* Fountain recycle = DispatchCompute step 6 (SPHFluid3D.cpp:519, DispatchFountainRecycle :526-544,
 * shaders/FountainRecycle.comp): while fountainMode is set every dispatch ends with the recycle
 * pass and advances fountainSeed.  sph_get_fountain returns the current values (seed included). */
void sph_fountain_default(SphFountain* out);             /* SPHFluid3D.h:161-168 initialisers */
int sph_set_fountain(SphEngine* e, const SphFountain* f);
int sph_get_fountain(const SphEngine* e, SphFountain* out);

/* River / stream mode = DispatchCompute step 5 (SPHFluid3D.cpp:511-516: DispatchTerrainConstraints :546-560,
 * DispatchChannelConstraint :562-578, DispatchStreamEmit :580-602 with shaders/TerrainConstraints.comp,
 * ChannelConstraint.comp, StreamEmit.comp): while riverMode is set and a heightfield has been given, every dispatch
 * ends with terrain collision, channel confinement and recycling (one fused kernel: each pass touches only its own
 * particle); the fountain step is then skipped (:519) and sph_reset spawns along the channel (:104-160).  Dead code in
 * the reference's scene (Scene0p.cpp:1660 is the only writer of riverMode), provided for completeness.
 * Single-GPU engines only (recycled particles jump across slabs). */
void sph_river_default(SphRiver* out);                   /* SPHFluid3D.h:171-196 initialisers */
/* SPHFluidGPU::GenerateRiverTerrain(int seed), SPHFluid3D.cpp:772-878, as a pure host function: reads
 * params->param_boxCenter / param_boxHalf and river->terrainW / terrainH; writes every other member of *river,
 * terrainW * terrainH floats into `heights` (terrainHeights) and param_gravityY = -120, param_gravityZ = 0 (:864-865).
 * std::rand() is the Microsoft runtime's LCG (the reference is a Visual Studio project). */
int sph_generate_river_terrain(SphParams* params, int seed, SphRiver* river, float* heights);
/* The river branch of InitializeParticles (:104-160) as a pure host function; writes exactly nRequested records. */
int sph_spawn_river_particles(const SphParams* params, const SphRiver* river, const float* heights, size_t nRequested,
                              uint32_t seed, SphParticle* out, size_t* nOut, float* massOut);
/* Members + heightfield into the engine (the glBufferData of terrainSSBO, :868-873).  heights == NULL keeps the
 * heightfield given before (terrainW / terrainH must then be unchanged). */
int sph_set_river(SphEngine* e, const SphRiver* river, const float* heights);
int sph_get_river(const SphEngine* e, SphRiver* out);

/* ---- data ------------------------------------------------------------------------ */
size_t sph_num_particles(const SphEngine* e);            /* particles.size() / GetNumFluids() */
int sph_grid_info(const SphEngine* e, SphGridInfo* out); /* gridSize*, numCells, gridMinV, cellSize */
/* glBufferData of the particle SSBO, SPHFluid3D.cpp:417-429 (n must equal sph_num_particles). */
int sph_upload_particles(SphEngine* e, const SphParticle* host, size_t n);
/* Read-back of the SSBO (the reference never reads back; needed for parity tests). Synchronises. */
int sph_download_particles(SphEngine* e, SphParticle* host, size_t n);
/* Device pointer of the 80-byte AoS in original order: the `ssbo` renderers bind
 * (Scene0p.cpp:1625,2627,3065,3142). Borrowed, read-only, invalidated by reset/destroy.
 * With SPH_OPT_AOS_MODE 1 (default) this call is what brings the records up to date (one
 * streaming kernel on the engine's stream, no synchronisation): call it once per frame,
 * before the draw, exactly where Scene0p binds the buffer; the contents then stay valid
 * until the next dispatch. */
int sph_device_particles(SphEngine* e, const SphParticle** devPtr);
/* Render-side export: one float4 (x, y, z, w) per particle in original order into a DEVICE buffer the
 * caller owns (e.g. a GL vertex buffer mapped through HIP-GL interop), replacing the renderers' reads of
 * binding 0 (shaders/fluidDepth.vert:16-24, particleImpostor.vert; Scene0p.cpp:1625,2627,3065).
 * wMode: 0 = 1.0, 1 = density, 2 = foam (padA), 3 = speed |vel|, 4 = dye (padB).  Asynchronous on the
 * engine's stream (work the caller has queued on OTHER streams for devOut4, e.g. a fill, is not ordered
 * against it: finish that first, or hand the engine the caller's stream at creation); n must equal
 * sph_num_particles. */
int sph_pack_render_buffer(SphEngine* e, float* devOut4, size_t n, int wMode);
/* Initial host-side records (SPHFluidGPU::particles: initial state only, never refreshed). */
int sph_initial_particles(const SphEngine* e, SphParticle* host, size_t n);
/* Grid as BuildGrid.comp defines it, for tests: cellCount[numCells] and
 * particleCell[n] (binding 3) in the reference's cell indexing. Synchronises. */
int sph_download_grid(SphEngine* e, int32_t* cellCount, size_t nCells, int32_t* particleCell, size_t n);
int sph_sync(SphEngine* e);
/* Diagnostic counters of the list passes k_sph_walk / k_sph_list (SPH_OPT_DEBUG bit 3), summed over launches since the last
 * reset, 8 slots: [0] candidate rows walked from global memory because the wave's window did not fit (k_sph_walk only),
 * [1] targets recomputed by an exact fallback sweep, [2] neighbour-list entries, [3] candidate rows (k_sph_walk only),
 * [4] lanes (one target each), [5] targets whose list overflowed, [6] targets that left the list's slack (sweep-3
 * fallback), [7] waves with at least one fallback target.  Never used on a timed path. */
int sph_debug_counters(SphEngine* e, uint64_t* out, int count, int reset);

/* ---- field sampling at probe points and on regular lattices (no reference counterpart) ------------------------------------------
 * The fields of the CURRENT state at arbitrary points.  A probe at x sees exactly the candidates sweep 1 of the SPH pass sees for a
 * particle at x: the members of the <= 27 cells around x's cell (BuildGrid's formula: (x - gridMin) / cellSize with IEEE division,
 * floorf, clamped to the grid), 9 rows in (dz, dy) order, each row one contiguous run of sorted slots, members ascending by id.  With
 * t_j = max(h^2 - r^2, 0), r^2 the fma-based dot3 of x - x_j:
 *   density  = mp6 * sum t_j^3, accumulated as dsum = fmaf(t*t, t, dsum) like sweep 1; NOT clamped (0 in empty space)
 *   count    = number of candidates with r^2 < h^2
 *   fraction = mp6 * sum invRho_j t_j^3 (Shepard sum, invRho_j = 1/rho_j of the sorted copy): ~1 inside the fluid, 0 outside
 *   vel, pressure = sum w_j v_j / sum w_j (the same for P), w_j = invRho_j t_j^3; 0 where sum w_j = 0
 * so fmaxf(density(x_i), rho0 / 2) at a fluid particle's position is, bit for bit, the density the next substep writes into its
 * record.  A probe with a non-finite coordinate gives an all-zero record.  mp6 = param_mass * poly6 coefficient.
 * Every call first builds the grid of the current state (compute_grid_extents, import, counting sort: about 150 us at 4 M particles,
 * timed under the bin / scan / scatter classes); the sampling kernel itself is timed as SPH_K_OTHER.  The next dispatch builds its own
 * grid: sampling never changes the simulation.  Refused with SPH_ERR_STATE: z-slab engines (their halo records after a step are the
 * step's entry state) and SPH_OPT_GRID_BUILD 1 (no sorted copy).  With no particles every result is zero. */
typedef struct SphSample {
    float density, fraction, pressure;
    uint32_t count;
    float vel[3];
    float pad;
} SphSample;                       /* 32 bytes */
enum { SPH_FIELD_DENSITY = 0, SPH_FIELD_FRACTION = 1, SPH_FIELD_PRESSURE = 2, SPH_FIELD_SPEED = 3 /* |vel| */, SPH_FIELD_ALL = 4 /* SphSample */ };
/* m probes of 4 floats (x, y, z, unused) in HOST memory -> m records in host memory.  Synchronises. */
int sph_sample_points(SphEngine* e, const float* points4, size_t m, SphSample* out);
/* The same with DEVICE arrays; asynchronous on the engine's stream. */
int sph_sample_points_device(SphEngine* e, const float* devPoints4, size_t m, SphSample* devOut);
/* Lattice points origin + (float)i * spacing per axis (an fp32 multiply, then an add), i < dims, x fastest, into a DEVICE buffer:
 * one float per point (SPH_FIELD_DENSITY / _FRACTION / _PRESSURE / _SPEED) or one SphSample per point (SPH_FIELD_ALL).  dims >= 1,
 * at most 2^31 - 1 points; spacing finite and > 0.  Asynchronous on the engine's stream. */
int sph_sample_lattice(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int field, void* devOut);

/* ---- iso-surface of a lattice as a closed triangle mesh (no reference counterpart) ------------------------------
 * Marching tetrahedra on the Kuhn (Freudenthal) split of the lattice origin + (float)i * spacing (x fastest, every dims >= 2, at most
 * 2^31 - 1 points).  A point is inside iff its value >= iso (NaN never is).  Each crossed lattice edge (from point a in one of the 7
 * directions x, y, xy, z, xz, yz, xyz) gets exactly one vertex, ordered by a's index, then direction; position pa + t (pb - pa) with
 * t = (iso - fa) / (fb - fa); normal -(ga + t (gb - ga)) normalised, g the central (one-sided on the lattice's first and last point)
 * difference of the values, (0, 0, 0) where it vanishes.  Triangles are ordered by cube, then tet, then table order, and wound so that
 * their normals point out of the inside region.  With no inside point on the lattice's outer layer the mesh is a closed, oriented
 * 2-manifold: every undirected edge in exactly two triangles.  The bits depend only on the values, iso, origin, spacing and dims.
 * Both extract calls synchronise once (to read the counts back), then queue the vertex and triangle kernels on the engine's stream
 * (timed as SPH_K_OTHER).  The returned device arrays are borrowed from the engine: valid until its next extract call, sph_reset or
 * sph_destroy; after a failed extract call the engine holds no surface.  An empty surface has counts 0 and null arrays.
 * SPH_ERR_ARG: a null argument, dims < 2 or more than 2^31 - 1 points, a spacing that is not finite and > 0, an iso that is not finite,
 * a field other than SPH_FIELD_DENSITY / _FRACTION / _PRESSURE / _SPEED.  SPH_ERR_CAPACITY: more than 2^32 - 1 vertices or triangles. */
typedef struct SphSurfaceVertex {
    float pos[3];
    float normal[3];
} SphSurfaceVertex;                /* 24 bytes */
typedef struct SphSurface {
    uint32_t numVertices, numTriangles;
    const SphSurfaceVertex* vertices;  /* device, borrowed */
    const uint32_t* triangles;         /* device, borrowed: 3 vertex indices per triangle */
} SphSurface;
/* Samples `field` of the current state on the lattice exactly as sph_sample_lattice does (into engine-owned scratch), then meshes it.
 * Refused with SPH_ERR_STATE where sampling is: z-slab engines and SPH_OPT_GRID_BUILD 1. */
int sph_extract_surface(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int field, float iso, SphSurface* out);
/* Meshes the caller's DEVICE array of dims[0] * dims[1] * dims[2] floats (x fastest).  Reads no particles: works on any engine. */
int sph_extract_surface_volume(SphEngine* e, const float* devValues, const float origin[3], const float spacing[3], const int dims[3], float iso,
                               SphSurface* out);
/* Copies the last extracted surface to HOST arrays (vertexCap records, triangleCap triangles of 3 indices).  Synchronises.
 * SPH_ERR_CAPACITY (nothing written) if a capacity is below the count; SPH_ERR_STATE if the engine holds no surface. */
int sph_surface_download(SphEngine* e, SphSurfaceVertex* vertices, size_t vertexCap, uint32_t* triangles3, size_t triangleCap);

/* ---- statistics of the particle state (no reference counterpart) -------------------------------------------------
 * Totals, extrema and histograms of the state the next dispatch would start from, reduced on the device.  The result is a pure function
 * of the 80-byte records sph_download_particles would return, the current members and the grid they imply.
 * Sets: fluid = isGhost == 0; active ghost = isGhost == 1 && isActive != 0; inactive ghost = isGhost == 1 && isActive == 0; other = the
 * rest.  A fluid record is non-finite if any of pos.xyz, vel.xyz, density, pressure, padA is not finite.  The COUNTED set is the finite
 * fluid records: everything except the counts is over it.  A counted record has escaped if floorf((p - gridMin) / cellSize) is < 0 or
 * >= the grid dimension on some axis (the unclamped cell index of BuildGrid).
 * Extrema compare with the fp32 <; of records that compare equal the lowest id wins and its stored bits are reported; an empty counted
 * set gives min +inf, max -inf, id 0xFFFFFFFF.  speed2 = (vx*vx + vy*vy) + vz*vz in fp32 without fma; maxSpeed = sqrtf(maxSpeed2.value).
 * Sums are fp64 (every fp32 value converted first, no fma), in a FIXED order: the slots in canonical order (cell ascending, id ascending
 * inside a cell; records outside the counted set contribute +0.0), tiles of 2048 slots reduced by pairwise halving
 * (x[i] += x[i + s], s = 1024 .. 1), the tile sums padded to a power of two and reduced by the same halving.  Terms: pos, vel,
 * (vx*vx + vy*vy) + vz*vz, density, density*density, pressure, padA (foam), 1.0 / density (0 where density <= 0), and
 * (pos - param_boxCenter) x vel (d = pos - c in fp64, then (dy*vz - dz*vy, dz*vx - dx*vz, dx*vy - dy*vx)).
 * Cell occupancy comes from the grid: occupancy[m] = cells with exactly m members (m < 64), occupancy[64] = cells with >= 64.
 * Histogram k of a field over the counted set has bins_k + 2 slots of uint64: v < lo -> slot 0, v >= hi -> slot bins + 1, otherwise
 * 1 + min((int)floorf((v - lo) * ((float)bins / (hi - lo))), bins - 1), all in fp32; SPH_STAT_SPEED bins sqrtf(speed2), SPH_STAT_FOAM padA.
 * Every call first builds the grid of the current state as sampling does (timed under the bin / scan / scatter classes); the statistics
 * kernels are timed as SPH_K_OTHER.  The next dispatch builds its own grid: a call never changes the simulation.
 * SPH_ERR_STATE (before any allocation): z-slab engines, SPH_OPT_GRID_BUILD 1.  SPH_ERR_ARG: a null output, nSpecs outside 0..4, null
 * specs or histogram output with nSpecs > 0, an unknown field, bins outside 1..1024, lo or hi not finite, lo >= hi, or a bin scale
 * (float)bins / (hi - lo) that is not finite in fp32.  With no particles: all-zero counts and sums, the empty-set extrema. */
typedef struct SphStatExtremum {
    float value;
    uint32_t id;                   /* particle id (index of the record) that attains it; 0xFFFFFFFF if none */
} SphStatExtremum;                 /* 8 bytes */
typedef struct SphStatistics {
    uint64_t numRecords, numFluid, numActiveGhosts, numInactiveGhosts, numOther, numNonFinite, numCounted, numEscaped;
    uint32_t firstNonFiniteId, firstEscapedId;          /* lowest id among them, 0xFFFFFFFF if none */
    SphStatExtremum minPos[3], maxPos[3], minDensity, maxDensity, minPressure, maxPressure, maxFoam, maxSpeed2;
    float maxSpeed;
    uint32_t reserved0;                                 /* 0 */
    double sumPos[3], sumVel[3], sumSpeed2, sumDensity, sumDensity2, sumPressure, sumFoam, sumInvDensity, sumAngular[3];
    uint64_t occupiedCells;
    uint32_t maxCellCount, maxCellIndex;                /* the largest member count of a cell and the lowest cell index that has it */
    uint64_t occupancy[65];
} SphStatistics;                   /* 832 bytes */
typedef struct SphHistogramSpec {
    int32_t field;                 /* SPH_STAT_* */
    uint32_t bins;                 /* 1 .. 1024 */
    float lo, hi;                  /* finite, lo < hi */
} SphHistogramSpec;                /* 16 bytes */
enum { SPH_STAT_DENSITY = 0, SPH_STAT_PRESSURE = 1, SPH_STAT_SPEED = 2, SPH_STAT_POS_X = 3, SPH_STAT_POS_Y = 4, SPH_STAT_POS_Z = 5, SPH_STAT_FOAM = 6 };
enum { SPH_STAT_MAX_SPECS = 4, SPH_STAT_MAX_BINS = 1024 };
/* Statistics into a HOST struct and HOST histograms (histogram k: bins_k + 2 consecutive uint64_t, in spec order).  `specs` is a host
 * array of nSpecs <= 4 entries (nSpecs == 0 with null specs / histOut is the common case).  Synchronises. */
int sph_statistics(SphEngine* e, SphStatistics* out, const SphHistogramSpec* specs, int nSpecs, uint64_t* histOut);
/* The same into a DEVICE struct and DEVICE histograms (`specs` stays a host array); asynchronous on the engine's stream. */
int sph_statistics_device(SphEngine* e, SphStatistics* devOut, const SphHistogramSpec* specs, int nSpecs, uint64_t* devHistOut);

/* ---- passive tracers advected inside the substep, with pathlines (no reference counterpart) ----------------
 * A tracer is a point that the fluid carries and that does not act on the fluid.  The engine holds M >= 0 tracers in the caller's order.
 * Let u(x) be the `vel` of the SphSample that sph_sample_points returns for a probe at x on the state a substep STARTS from, and phi(x)
 * its `fraction` (same candidates, same order, same fma placement, zero where sum w_j = 0, all-zero for a non-finite x).  One substep with
 * time step dt (overrideDt if > 0, else param_timeStep) moves every tracer, per axis, in fp32, with a multiply and then an add (no fma):
 *   SPH_TRACER_EULER     v = u(x);                                          x' = x + dt * v
 *   SPH_TRACER_MIDPOINT  v1 = u(x); xm = x + (0.5f * dt) * v1; v = u(xm);   x' = x + dt * v     (both on the same frozen entry state)
 * and then stores vel = v, fraction = phi(x) (at the position BEFORE the move: was the tracer in the fluid), age' = age + dt (one fp32
 * add).  A tracer with a non-finite coordinate keeps its position bits, gets vel = 0, fraction = 0 and still ages.  A tracer outside
 * the fluid (sum w_j = 0) does not move; one outside the grid takes the clamped cell, as a probe does.  Records whose density is <= 0
 * (spawned or uploaded records before their first substep) have 1/rho = 0, so u = 0 and phi = 0 there: tracers do not move during
 * the FIRST substep on such a state.
 * Hence the tracers after n substeps are, bit for bit, what the loop  s = sample(x); dispatch(dt); x = x + dt * s.vel  gives (two
 * samples per substep for the midpoint rule), and the particle records are byte-identical with and without tracers.
 * Tracers see the entry state of the substep, before the fountain / river recycle of that dispatch.  param_pause: no substep, no
 * move, no ageing.  Impulses, sph_upload_particles and sph_set_params do not touch tracers; sph_reset drops the set, sph_destroy
 * frees it.  The advection runs behind the substep's own grid build (no second build), under sph_dispatch_n and inside its captured
 * graphs, timed as SPH_K_OTHER.  With no tracers set a dispatch launches exactly what it launched before.
 * Pathline history: historyCap K >= 0 snapshots, one every historyStride S >= 1 substeps.  With c the substeps that have advected the
 * current set (0 right after a set call), snapshot q holds (x, y, z, age) of all M tracers after substep c = q S; snapshot 0 is the
 * seed; snapshot q lives in slot q mod K of a device ring of K M float4.  min(c / S + 1, K) snapshots are stored.
 * SPH_ERR_STATE from the set calls, before anything is allocated, on z-slab engines and under SPH_OPT_GRID_BUILD 1; setting
 * SPH_OPT_GRID_BUILD 1 while tracers exist makes the next dispatch fail with SPH_ERR_STATE and move nothing.  SPH_ERR_ARG: null
 * pointers with m > 0, unknown integrator, historyStride == 0, historyCap * m above 2^31 - 1 float4. */
typedef struct SphTracer { float pos[3]; float age; float vel[3]; float fraction; } SphTracer;   /* 32 bytes */
enum { SPH_TRACER_EULER = 0, SPH_TRACER_MIDPOINT = 1 };
/* m points of 4 floats (x, y, z, initial age) in HOST memory replace the engine's tracer set; m == 0 drops it.  Synchronises. */
int sph_tracers_set(SphEngine* e, const float* points4, size_t m, int integrator, uint32_t historyCap, uint32_t historyStride);
/* The same from a DEVICE array, asynchronous on the engine's stream. */
int sph_tracers_set_device(SphEngine* e, const float* devPoints4, size_t m, int integrator, uint32_t historyCap, uint32_t historyStride);
size_t sph_tracers_count(const SphEngine* e);
/* c, the number of stored snapshots and the number q of the oldest stored one (any pointer may be null). */
int sph_tracers_info(const SphEngine* e, uint64_t* substeps, uint32_t* snapshots, uint64_t* firstSnapshot);
/* m records in the caller's order to HOST memory (cap >= m, else SPH_ERR_CAPACITY, nothing written).  Synchronises. */
int sph_tracers_download(SphEngine* e, SphTracer* out, size_t cap);
/* Borrowed DEVICE pointer to the m records in the caller's order, valid until the next dispatch, set, reset or destroy; no synchronisation. */
int sph_tracers_device(SphEngine* e, const SphTracer** devPtr);
/* The stored snapshots, oldest first, to HOST memory: snapshotCap * m * 4 floats (snapshotCap >= the stored count, else
 * SPH_ERR_CAPACITY).  SPH_ERR_STATE without a history (K == 0 or no tracers).  Synchronises. */
int sph_tracers_history(SphEngine* e, float* out4, size_t snapshotCap, uint32_t* snapshotsOut, uint64_t* firstSnapshotOut);

/* ---- diffusing scalar fields carried by the particles: dye, heat (no reference counterpart) ----------------
 * The engine holds K channels, 1 <= K <= SPH_MAX_SCALAR_CHANNELS, one fp32 each per particle, stored particle-major (c[i * K + k])
 * in the caller's order: index i is the same particle forever, like the records.  A value moves with its particle for free and
 * exchanges with the particle's neighbours through an SPH Laplacian (Brookshaw / Cleary-Monaghan with the spiky gradient the force
 * sweep uses).  Channel k has a diffusivity D_k >= 0 and a decay rate lambda_k >= 0; `coeffs` is always 2 K floats,
 * D_0 .. D_{K-1} and then lambda_0 .. lambda_{K-1}.
 * One non-paused substep with time step dt (overrideDt if > 0, else param_timeStep) updates every target i from the state the
 * substep STARTS from -- the sorted copy (x, y, z, 1/rho) the tracers and the SPH pass read; 1/rho = 0 for a record with density <= 0:
 *   targets      records with isGhost == 0, finite position and 1/rho_i > 0; every other record keeps its values bit for bit.  Ghost
 *                records are neither targets nor candidates (the gather step gives them the weight 0), so the exchange is conservative.
 *   candidates   those of a probe of sph_sample_points at x_i: the clamped cell of x_i, 9 rows in (dz, dy) order, slots ascending
 *                (members of a cell ascending by index); particle i itself is skipped.
 *   pairs        those with 0 < r2 < h2 and 1/rho_j > 0, r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of d = x_i - x_j, h2 = h * h.
 *   weight       r = sqrtf(r2); u = h - r; G = ((u * u) * r) / (r2 + 0.01f * h2); w = ((1/rho_i) * (1/rho_j)) * G   (bitwise symmetric in i, j)
 *   sums         a_k = fmaf(w, c_jk - c_ik, a_k); W = W + w          (both start at +0, candidates in the order above)
 *   finish       kLap = (float)(90 m / (pi ((h^2 h^2) h^2))) with m = param_mass, h = param_h, in double;
 *                c_ik' = c_ik + dt * (((D_k * kLap) * a_k) - (lambda_k * c_ik))      (fp32 multiplies and adds, no fma)
 *   number       s_i = (dt * (Dmax * kLap)) * W with Dmax = max_k D_k.  The engine keeps the maximum of s_i over the targets of the last
 *                substep, taken on the float's bits (non-negative floats order as unsigned integers), so it does not depend on launch
 *                shape.  Explicit Euler keeps a maximum principle only while s_i + dt lambda_k <= 1; the engine reports, it does not clamp.
 * Records whose density is <= 0 (before their first substep) have 1/rho = 0: nothing diffuses during the FIRST substep on such a
 * state, as tracers do not move then.  D is the operator's nominal coefficient.  The weight carries 1 / (rho_i rho_j), so D is rho times
 * a diffusivity (Cleary-Monaghan's conductivity over heat capacity): a long mode of wave number k decays at f (D / rho) k^2, and the
 * factor f depends on the neighbours per support (0.92 on a cubic lattice of spacing h / 2, 0.30 at 0.85 h).
 * Recycled particles (fountain, river) keep their values.  param_pause: no step.  sph_upload_particles, impulses and sph_set_params do
 * not touch scalars (kLap follows param_mass and param_h of the dispatch); sph_reset drops them, sph_destroy frees them.  The particle
 * records are byte-identical with and without scalars, padB included; with no scalars set a dispatch launches exactly what it launched
 * before.  The step runs behind the substep's own grid build as two launches (gather, sweep), under sph_dispatch_n and inside its
 * captured graphs, timed as SPH_K_OTHER.  Set, drop and the channel count enter a graph's key; the coefficients live in device memory,
 * so a replayed graph sees a later sph_scalars_set_coefficients.
 * SPH_ERR_STATE from the set calls, before anything is allocated, on z-slab engines and under SPH_OPT_GRID_BUILD 1; setting
 * SPH_OPT_GRID_BUILD 1 while scalars exist makes the next dispatch fail with SPH_ERR_STATE and change nothing.  SPH_ERR_ARG (the
 * previous state stays): a null pointer where data is required, n != sph_num_particles, K outside 1 .. 4, a non-finite or negative
 * coefficient, a channel out of range, an unknown mode, a radius that is not finite and > 0. */
#define SPH_MAX_SCALAR_CHANNELS 4
enum { SPH_SCALAR_SET = 0, SPH_SCALAR_ADD = 1 };
/* n * channels floats in HOST memory replace the engine's scalar set; channels == 0 drops it (values, coeffs ignored).  values == NULL
 * seeds channel 0 from padB of the current records (the reference's dye) and the other channels with 0.  Synchronises. */
int sph_scalars_set(SphEngine* e, const float* values, size_t n, int channels, const float* coeffs);
/* The same from a DEVICE array (`coeffs` stays a host array), asynchronous on the engine's stream. */
int sph_scalars_set_device(SphEngine* e, const float* devValues, size_t n, int channels, const float* coeffs);
/* New D_k and lambda_k for the current channels, stream-ordered: substeps enqueued later, replayed graphs included, use them. */
int sph_scalars_set_coefficients(SphEngine* e, const float* coeffs);
int sph_scalars_channels(const SphEngine* e);
/* n * K floats in the caller's order to HOST memory (cap >= n * K floats, else SPH_ERR_CAPACITY, nothing written).  Synchronises. */
int sph_scalars_download(SphEngine* e, float* out, size_t cap);
/* Borrowed DEVICE pointer to the n * K floats (NULL without scalars), valid until the next dispatch, set, reset or destroy; no synchronisation. */
int sph_scalars_device(SphEngine* e, const float** devPtr);
/* The dye injector and the heat source: channel = value (SPH_SCALAR_SET) or channel += value (SPH_SCALAR_ADD, one fp32 add) for every
 * non-ghost record whose CURRENT position lies strictly inside the sphere: fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < radius * radius with
 * d = x - center (a particle exactly on the sphere is not inside, nor is one with a non-finite coordinate).  One per-particle kernel on
 * the engine's own state arrays, stream-ordered; no record is materialised. */
int sph_scalars_paint(SphEngine* e, const float center[3], float radius, int channel, float value, int mode);
/* The substeps stepped since the set call and the diffusion number of the last one (0 before the first); either pointer may be null.
 * Synchronises when the number is asked for. */
int sph_scalars_info(SphEngine* e, uint64_t* substepsOut, float* maxNumberOut);
/* Per channel over the targets of the state the next dispatch would start from (non-ghost, finite position, density > 0) whose value is
 * finite: count, fp64 sum and sum of squares (each value converted to fp64 first, the square one exact fp64 product) in the FIXED order
 * of sph_statistics (slots in canonical order, tiles of 2048 by pairwise halving, the tile sums by the same halving), and the extrema
 * with the lowest id among equals (empty set: +inf, -inf, id 0xFFFFFFFF).  It is the statistics reduction run over each channel, behind a
 * grid build of the current state; K records to HOST memory.  Synchronises. */
typedef struct SphScalarMoments {
    uint64_t count;
    double sum, sumSquares;
    SphStatExtremum min, max;
} SphScalarMoments;                /* 40 bytes */
int sph_scalars_moments(SphEngine* e, SphScalarMoments* out);
/* Shepard value of one channel, sum w_j c_jk / sum w_j, with the w_j = ((t t) t) (1/rho_j), the candidates and the order of
 * sph_sample_points (num = fmaf(w_j, c_jk, num), wsum = wsum + w_j, one IEEE division): 0 where sum w_j = 0 and for a non-finite point.
 * m points of 4 floats (x, y, z, unused) -> m floats.  Host arrays: synchronises.  Device arrays: asynchronous on the engine's stream. */
int sph_scalars_sample_points(SphEngine* e, const float* points4, size_t m, int channel, float* out);
int sph_scalars_sample_points_device(SphEngine* e, const float* devPoints4, size_t m, int channel, float* devOut);
/* The same on the lattice origin + (float)i * spacing of sph_sample_lattice (x fastest) into a DEVICE array of one float per point: it
 * feeds sph_extract_surface_volume unchanged (concentration iso-surfaces).  Asynchronous on the engine's stream. */
int sph_scalars_sample_lattice(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int channel, float* devOut);
/* Host-only bit-level yardstick: one substep's scalar update of `values` (n * channels floats, in place) on the state `particles`, with
 * the same pair and finish functions in plain loops over a grid built as the counting sort builds it.  dt <= 0: param_timeStep. */
int sph_scalars_step_host(const SphParticle* particles, size_t n, const SphParams* params, float dt, float* values, int channels,
                          const float* coeffs, float* maxNumberOut);

/* ---- kinematic solid obstacles with fluid force and torque feedback (no reference counterpart) ----------
 * Up to SPH_MAX_OBSTACLES rigid bodies whose motion the caller prescribes.  Every substep, after the SPH pass and the container and
 * before the river / fountain step, each non-ghost particle with finite coordinates meets bodies 0..K-1 in order: a particle strictly
 * inside a body is projected onto its surface and, if it moves into the surface (u_n < 0 relative to the surface velocity
 * V + omega x (p' - c)), gets the body's wall response.  The engine sums, per body, the linear impulse J = m (v - v') and the angular
 * impulse (p' - c) x J in fp64 (the fluid's push on the body, about its centre), and then advances every pose by one substep on the
 * device: c += dt V, q = normalize(q + (dt / 2) (0, omega) q) when omega != 0.  Bodies do not react to the fluid.  The sums are
 * independent of launch shape, AoS mode, pass kernel and graph replay.  With no obstacles a dispatch launches exactly what it launched
 * before.  SPH_ERR_ARG (the previous set stays): unknown shape, a used size component not finite or <= 0, a zero or non-finite
 * quaternion (or one whose fp32 squared norm is not a finite positive number), any non-finite field, restitution or friction outside [0, 1], count above SPH_MAX_OBSTACLES, index out of range.
 * SPH_ERR_STATE: z-slab engines.  param_pause: nothing moves, nothing accumulates. */
#define SPH_MAX_OBSTACLES 16
enum { SPH_OBSTACLE_SPHERE = 0, SPH_OBSTACLE_BOX = 1, SPH_OBSTACLE_CAPSULE = 2 };
typedef struct SphObstacle {       /* 76 bytes */
    int32_t  shape;
    float    size[3];      /* sphere: x = radius | box: half extents | capsule: x = radius, y = half length of the core segment along local y */
    float    center[3];    /* world */
    float    rotation[4];  /* unit quaternion (w, x, y, z), local -> world; normalised by the engine on set */
    float    vel[3];       /* world units / s */
    float    omega[3];     /* rad / s, world frame, about center */
    float    restitution;  /* default 0.15, param_wallRestitution's default */
    float    friction;     /* default 0.02, param_wallFriction's default */
} SphObstacle;
/* A sphere of radius 1 at the origin, identity rotation, at rest, default coefficients. */
void sph_obstacle_default(SphObstacle* out);
/* Replaces the set (count 0 clears it and frees its buffers).  Stream-ordered, no synchronisation.  The accumulators survive a set with
 * the same count and are zeroed by a set with another count. */
int  sph_obstacles_set(SphEngine* e, const SphObstacle* obs, int count);
/* New linear / angular velocity of body `index`; keeps the pose the device holds.  Stream-ordered, no synchronisation. */
int  sph_obstacles_set_motion(SphEngine* e, int index, const float vel[3], const float omega[3]);
/* The current (advanced) bodies to HOST memory (cap >= count, else SPH_ERR_CAPACITY); countOut may be null.  Synchronises. */
int  sph_obstacles_get(SphEngine* e, SphObstacle* out, int cap, int* countOut);
/* (Jx, Jy, Jz, Lx, Ly, Lz) per body (cap >= count, else SPH_ERR_CAPACITY), the simulated time (fp64 sum of dt) and the substeps summed
 * since the last zeroing; reset != 0 zeroes them after the read.  sph_reset zeroes them too (it keeps the set and the poses).  Any
 * output pointer may be null.  Synchronises. */
int  sph_obstacles_impulses(SphEngine* e, double* out6, int cap, double* timeOut, uint64_t* substepsOut, int reset);
/* Host-only, no device: the same __host__ __device__ functions the kernel runs.  The rotation is used as given (pass a pose
 * sph_obstacles_get returned, or one normalised as section 3e does).  apply: one obstacle step on n records in index order, impulses6
 * (count x 6, may be null) receives the sums in index order.  advance: one pose advance of every body by dt, in place. */
int  sph_obstacles_apply_host(const SphObstacle* obs, int count, float particleMass, SphParticle* particles, size_t n, double* impulses6);
int  sph_obstacles_advance_host(SphObstacle* obs, int count, float dt);

/* ---- triangle-mesh obstacles through signed distance lattices (no reference counterpart) ---------------
 * A VOLUME is an engine-owned lattice of fp32 signed distances in a body's local length unit, NEGATIVE INSIDE the solid, x fastest,
 * centred on the body: local coordinate of point i on axis a is (float)i * spacing_a - half_a, half_a = 0.5f (float)(dims_a - 1)
 * spacing_a.  Up to SPH_MAX_VOLUMES exist per engine.  Bound to a body of shape SPH_OBSTACLE_BOX (whose box stays what it is for the
 * cull and for the host entry points of the block above), the volume makes the solid box, lattice extent and {phi < 0} intersected:
 * a particle strictly inside the box whose lattice coordinate lies in the extent and whose trilinear phi is < 0 is projected by two
 * steps o <- o - phi(o) grad phi(o) / |grad phi(o)| (the gradient of the same trilinear interpolant; the second evaluation at the
 * point clamped into the extent), the local normal is the unit gradient of the second evaluation, and where a gradient has length 0
 * or is not finite the box's nearest face decides.  Everything else (surface velocity, response, impulses, pose advance) is the
 * block above.  Users normally give the box size = half (sph_volume_info).  Bindings and the volume table live in device memory: a
 * replayed graph sees a later bind.  With no body bound a dispatch launches exactly the kernels it launches without volumes.
 * SPH_ERR_ARG (nothing changes): null pointers, a dimension < 2, more than 2^31 - 1 points, a spacing not finite or <= 0, an id that
 * names no volume, an index outside the set, a body that is not a box.  SPH_ERR_CAPACITY: all slots in use.  SPH_ERR_STATE: z-slab
 * engines; sph_volume_destroy of a bound volume. */
#define SPH_MAX_VOLUMES 16
/* Copies dims[0] dims[1] dims[2] floats from host (onDevice == 0; synchronises) or device (stream-ordered) memory; *idOut is the slot. */
int  sph_volume_create(SphEngine* e, const float* values, const int dims[3], const float spacing[3], int onDevice, int* idOut);
/* Frees the slot.  Synchronises. */
int  sph_volume_destroy(SphEngine* e, int id);
/* Any output pointer may be null. */
int  sph_volume_info(SphEngine* e, int id, int dimsOut[3], float spacingOut[3], float halfOut[3]);
/* Binds volume `id` to body `index` (id < 0 unbinds).  sph_obstacles_set clears every binding (a set replaces the set);
 * sph_obstacles_set_motion keeps them.  Stream-ordered, no synchronisation. */
int  sph_obstacles_bind_volume(SphEngine* e, int index, int id);
/* The volume bound to body `index`, -1 if none. */
int  sph_obstacles_volume(SphEngine* e, int index, int* idOut);
/* Host-only, no device: the same __host__ __device__ functions the kernels run.  sample: phi and the gradient of the trilinear
 * interpolant (divided by the spacing, not normalised) at a local point; *insideOut = 1 iff the point lies in the extent and phi < 0;
 * outside the extent (or at a NaN coordinate) phi is a quiet NaN and the gradient zero.  apply: sph_obstacles_apply_host with body b
 * bound to volumes[bindings[b]] (bindings[b] < 0: none; bound bodies must be boxes); with every binding < 0 the result equals
 * sph_obstacles_apply_host byte for byte. */
typedef struct SphVolumeHost {     /* 32 bytes */
    const float* values;
    int          dims[3];
    float        spacing[3];
} SphVolumeHost;
int  sph_volume_sample_host(const float* values, const int dims[3], const float spacing[3], const float local[3], float* phiOut, float gradOut[3],
                            int* insideOut);
int  sph_obstacles_apply_host_volumes(const SphObstacle* obs, int count, const SphVolumeHost* volumes, int volumeCount, const int* bindings,
                                      float particleMass, SphParticle* particles, size_t n, double* impulses6);
/* Signed distance from every lattice point origin + (float)i * spacing (x fastest) to a triangle mesh given in HOST memory (3 floats per
 * vertex, 3 uint32 per triangle), one float per point into the caller's DEVICE array; asynchronous on the engine's stream after the mesh
 * upload.  Reads no particles: works on any engine.  Magnitude: sqrtf of the minimum over the triangles of the squared distance to the
 * closest point of the triangle (bit-exact, independent of how the work is split).  Sign: negative where the generalised winding number
 * of the mesh is >= 0.5.  Triangles are counter-clockwise seen from outside (what sph_extract_surface emits); a closed mesh wound the
 * other way is OUTSIDE everywhere.  Timed as SPH_K_OTHER.  SPH_ERR_ARG: null pointers, nt == 0, an index >= nv, a vertex or origin
 * that is not finite, a dimension < 1, more than 2^31 - 1 points, a spacing not finite or <= 0.  The _host twin runs the same per-pair functions in plain loops into host memory. */
int  sph_mesh_distance(SphEngine* e, const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float origin[3],
                       const float spacing[3], const int dims[3], float* devOut);
/* sph_mesh_distance straight into a new volume: the lattice of dims points is centred on `center` (origin = center - half), so a body
 * of shape SPH_OBSTACLE_BOX at `center` with size = half (sph_volume_info) bound to *idOut is the mesh as an obstacle.  Nothing leaves the device. */
int  sph_volume_from_mesh(SphEngine* e, const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float center[3],
                          const float spacing[3], const int dims[3], int* idOut);
int  sph_mesh_distance_host(const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float origin[3], const float spacing[3],
                            const int dims[3], float* out);

/* ---- dynamic rigid bodies: obstacles moved by the fluid (no reference counterpart) ---------------------
 * A body of the obstacle set with a dynamics record is DYNAMIC: at the end of every substep the engine, on the device, turns the
 * substep's own sums (J, L) of that body into new velocities and advances the pose with them:
 *   o = M com, L_g = L - o x J (fp64), V_g = V + omega x o;  V_g += (float)(J / mass) + dt (gravityScale g + force / mass);
 *   omega += I_w^-1 (L_g + dt (torque - omega x (I_w omega))), I_w = M I M^T;  damping;  container contact (flag bit 0);
 *   V = V_g - omega x o;  the pose advance of section 3e with the new V and omega.
 * The particle pass of a substep sees the velocities the substep began with.  Container contact runs against the oriented box of
 * param_boxCenter, param_boxEulerDeg and the effective half extents (for param_shapeType 0 the container itself, for the other
 * shapes only their bounding box): support points (sphere: centre, radius R | capsule: the two ends of the core segment, radius r |
 * box: the eight corners, radius 0) against faces -x, +x, -y, +y, -z, +z; a penetrating point that moves into the face gets the normal
 * impulse j = -(1 + param_wallRestitution) v_n / (1 / mass + n . ((I_w^-1 (r x n)) x r)); no friction; afterwards the centre moves
 * inward by each face's largest penetration.  A body without a record is kinematic, exactly as before; the accumulators keep summing
 * what the fluid gave each body.  No body-body contact, no implicit coupling.  The exact operation order is DESIGN.md section 3g.
 * sph_obstacles_set clears every record (a set replaces the set); sph_obstacles_set_motion on a dynamic body is a kick; sph_reset
 * keeps the records.  SPH_ERR_ARG (the previous state stays): a non-finite field, mass <= 0, an inertia that is not positive
 * definite, a damping < 0, an index out of range, a null pointer where a record is required.  SPH_ERR_STATE: z-slab engines. */
#define SPH_DYNAMICS_CONFINED 1u
typedef struct SphObstacleDynamics {   /* 80 bytes */
    float    mass;             /* > 0 */
    float    inertia[6];       /* xx, yy, zz, xy, xz, yz about the centre of mass, body frame; positive definite */
    float    com[3];           /* centre of mass in the body frame, relative to center */
    float    gravityScale;     /* times param_gravity*, default 1 */
    float    force[3];         /* constant, world frame */
    float    torque[3];        /* constant, world frame */
    float    linearDamping;    /* per second: V *= max(0, 1 - linearDamping dt) */
    float    angularDamping;
    uint32_t flags;            /* SPH_DYNAMICS_CONFINED */
} SphObstacleDynamics;
/* mass 1, inertia diag(1, 1, 1), com 0, gravityScale 1, no force, torque or damping, confined by the container. */
void sph_obstacle_dynamics_default(SphObstacleDynamics* out);
/* Makes body `index` dynamic (dyn == NULL: kinematic again, keeping its current velocities).  Stream-ordered, no synchronisation. */
int  sph_obstacles_set_dynamics(SphEngine* e, int index, const SphObstacleDynamics* dyn);
/* The record of body `index` as set (*dynamicOut = 0 and a default record for a kinematic body).  Either output may be null. */
int  sph_obstacles_get_dynamics(SphEngine* e, int index, SphObstacleDynamics* out, int* dynamicOut);
/* Host-only, no device: the body step of one substep for `count` bodies, in place.  dyn[i].mass == 0 marks body i kinematic (it only
 * advances); impulses6 holds the substep's (J, L) per body (null: zeros); params supplies gravity, the container box and
 * param_wallRestitution.  The rotation is used as given, as in sph_obstacles_advance_host. */
int  sph_obstacles_step_host(SphObstacle* obs, const SphObstacleDynamics* dyn, int count, const double* impulses6, const SphParams* params, float dt);
/* Moments of the solid a volume describes, out = cell volume times the sum over the lattice points of w {1, x, y, z, xx, yy, zz, xy,
 * xz, yz}: x, y, z the fp32 local coordinates of section 3f widened to fp64, w = clamp(0.5 - phi / D, 0, 1) in fp32 with D the
 * cell diagonal.  A grid-sized reduction on the device without float atomics (the bits depend on the lattice only), timed as
 * SPH_K_OTHER.  Synchronises.  The _host twin runs the same per-point function in plain loops, points in ascending order. */
int  sph_volume_moments(SphEngine* e, int id, double out[10]);
int  sph_volume_moments_host(const float* values, const int dims[3], const float spacing[3], double out[10]);

/* ---- active scalars: buoyancy from heat or salt, and continuous sources (no reference counterpart) ----------
 * The scalar channels act back on the fluid, and regions in the world or riding on an obstacle feed them every substep on the device.
 * Both are off by default and belong to the scalar set: sph_scalars_set / _set_device reset them to none (and zero the books), sph_reset
 * drops them, sph_destroy frees them.  With neither set a dispatch launches exactly what it launched before.
 * One non-paused substep with time step dt (the dt the dispatch steps with) runs, on the substep's OUTPUT state, after the SPH pass, the
 * container and the obstacle step, and before river / fountain: the sources 0 .. S-1 in order, then the buoyancy kick.  Targets are
 * the records with isGhost == 0 and finite position; every other record keeps its bits and its values.
 *   frame      body == -1: d = p - center (world axes).  body == b: the local frame of obstacle b as the device holds it AFTER this
 *              substep's obstacle step (kinematic, volume-bound and dynamic bodies alike): q = p - c_b, l_a = fmaf(q_z, M_za, fmaf(q_y, M_ya,
 *              q_x * M_xa)) (l = M^T q, the dot3 of section 3e), d = l - center.
 *   inside     strict: sphere fmaf(d_z, d_z, fmaf(d_y, d_y, d_x * d_x)) < size[0] * size[0]; box |d_a| < size[a] on all three axes.
 *   hit        a target inside whose value c in the source's channel is finite.  Each source sees the result of the ones before it.
 *   arithmetic fp32, a multiply and then an add, no fma:  SPH_SOURCE_RATE  c' = c + dt * rate;
 *              SPH_SOURCE_RELAX  a = fminf(dt * rate, 1.0f); r = c + a * (target - c);
 *              c' = fminf(fmaxf(r, fminf(c, target)), fmaxf(c, target))   (the clamp only acts where a rounding of target - c would carry r
 *              past the target: c' never leaves the closed interval between c and target, so no stability number is needed)
 *   books      per source the number of (particle, substep) hits and the fp64 sum of (double)c' - (double)c (one fp64 subtraction per
 *              hit), cumulative since the last zeroing; with them the simulated time (fp64 sum of dt) and the substeps, which advance
 *              while at least one source is set, graph replays included.  No float atomic: the sums depend on the slot order of the
 *              state only.  A set call with another source count zeroes the books, one with the same count keeps them.
 *   buoyancy   s = 0; for k = 0 .. K-1: s = fmaf(beta_k, c_k - ref_k, s), on the values the sources just wrote.  Where s is finite and
 *              != 0: v_a' = v_a - (dt * s) * g_a per axis with g = (param_gravityX, Y, Z) of this dispatch (a multiply, a multiply and a
 *              subtract, no fma); otherwise the record is not written.  beta > 0 with c > ref accelerates against gravity (heat);
 *              salt takes beta < 0.  Positions are not touched and the velocity is not capped: the next pass's own cap applies.
 * The coefficients, the source table and the source count live in device memory: a replayed graph sees a later set call.  Whether the
 * kernels run, and their buffers, enter a graph's key.  While a beta is non-zero the SPH pass does not keep the 80-byte array current
 * by itself (SPH_OPT_AOS_MODE 0 writes it back after the substep, as with obstacles); sources alone never change a record.
 * SPH_ERR_STATE: no scalars; z-slab engines and SPH_OPT_GRID_BUILD 1 (as the block above); a dispatch while a source's body is >= the
 * obstacle count (the dispatch fails and changes nothing).  SPH_ERR_ARG (the previous state stays): a count above
 * SPH_MAX_SCALAR_SOURCES, a null pointer where data is needed (beta without ref), an unknown shape or mode, a channel outside [0, K), a
 * non-finite field, a used size component that is not > 0, rate < 0, body < -1 or >= SPH_MAX_OBSTACLES. */
#define SPH_MAX_SCALAR_SOURCES 8
enum { SPH_SOURCE_SPHERE = 0, SPH_SOURCE_BOX = 1 };
enum { SPH_SOURCE_RATE = 0, SPH_SOURCE_RELAX = 1 };
typedef struct SphScalarSource {   /* 64 bytes */
    int32_t  shape;        /* SPH_SOURCE_SPHERE | SPH_SOURCE_BOX */
    int32_t  channel;
    int32_t  mode;         /* SPH_SOURCE_RATE | SPH_SOURCE_RELAX */
    int32_t  body;         /* -1: world frame | b: local frame of obstacle b */
    float    center[3];
    float    size[3];      /* sphere: x = radius | box: half extents */
    float    rate;         /* RATE: value per second | RELAX: 1 / s */
    float    target;       /* RELAX only */
    float    pad[4];
} SphScalarSource;
/* K floats each (beta_k, ref_k), all finite; NULL, NULL switches buoyancy off.  Stream-ordered, no synchronisation. */
int  sph_scalars_set_buoyancy(SphEngine* e, const float* beta, const float* ref);
/* The coefficients as set (zeros while off); either pointer may be null. */
int  sph_scalars_get_buoyancy(SphEngine* e, float* beta, float* ref);
/* A unit sphere at the world origin on channel 0, SPH_SOURCE_RATE with rate 0. */
void sph_scalar_source_default(SphScalarSource* out);
/* Replaces the source table; count 0 clears it.  Stream-ordered, no synchronisation. */
int  sph_scalars_set_sources(SphEngine* e, const SphScalarSource* sources, int count);
/* The sources as set (cap >= count, else SPH_ERR_CAPACITY); countOut may be null. */
int  sph_scalars_get_sources(SphEngine* e, SphScalarSource* out, int cap, int* countOut);
/* The books: per source the fp64 sum and the hits (cap >= count, else SPH_ERR_CAPACITY), the simulated time and the substeps summed
 * since the last zeroing; reset != 0 zeroes them after the read.  Any output pointer may be null.  Synchronises. */
int  sph_scalars_injected(SphEngine* e, double* sums, uint64_t* hits, int cap, double* timeOut, uint64_t* substepsOut, int reset);
/* Host-only, no device: the same __host__ __device__ functions the kernel runs, on n records and n * channels values in place, in
 * index order (record i owns values[i * channels ..]).  beta, ref: NULL, NULL for no buoyancy.  obstacles: the poses a body-bound source
 * rides on, rotation used as given (pass what sph_obstacles_get returned).  sumsOut / hitsOut (nSources each, may be null) receive this
 * step's books, the sums added in index order.  dt <= 0: param_timeStep.  param_pause: nothing happens. */
int  sph_scalars_couple_host(SphParticle* particles, size_t n, const SphParams* params, float dt, float* values, int channels,
                             const float* beta, const float* ref, const SphScalarSource* sources, int nSources,
                             const SphObstacle* obstacles, int nObstacles, double* sumsOut, uint64_t* hitsOut);

/* ---- flow gates: what crosses a plane, counted inside the substep (no reference counterpart) ----------------
 * A gate is an oriented planar patch fixed in the world: a rectangle or an ellipse with centre `center` and the half-extent vectors u
 * and v (orthogonal, any length), or with SPH_GATE_UNBOUNDED its whole plane.  The forward normal is N = cross(u, v), per component a
 * multiply, a multiply and a subtract, not normalised.  Off by default; with no gates set a dispatch launches exactly what it launched
 * before.  One non-paused substep books, on its OUTPUT state, after the container, the obstacle step and the coupling step and before
 * river / fountain (a recycled particle's jump is never a crossing), for every record with isGhost == 0 whose position is finite at the
 * entry and at the exit of the substep (p0, p1), per gate, in fp32 with dot3(a, b) = fmaf(a_z, b_z, fmaf(a_y, b_y, a_x * b_x)):
 *   side     s0 = dot3(p0 - center, N), s1 = dot3(p1 - center, N); forward: s0 < 0 && s1 >= 0; backward: s0 >= 0 && s1 < 0; else nothing
 *   where    t = s0 / (s0 - s1); x_a = fmaf(t, p1_a - p0_a, p0_a); d = x - center; a = dot3(d, u); b = dot3(d, v);
 *            rectangle: |a| < dot3(u, u) && |b| < dot3(v, v); ellipse: fa = a / dot3(u, u), fb = b / dot3(v, v), fmaf(fa, fa, fb * fb) < 1;
 *            SPH_GATE_UNBOUNDED: always
 *   books    per gate the forward and backward counts, the fp64 sums of +(double)v_a (forward) / -(double)v_a (backward) of the output
 *            velocity, and of +-(double)c_k of the scalar channels after this substep's sources (a non-finite value adds 0, channels the
 *            engine does not carry stay 0); with them the simulated time (fp64 sum of dt) and the substeps since the last zeroing.  No
 *            float atomic: the sums depend on the slot order of the state only, the counts are exact.
 *   history  every `stride` substeps (counted since the ring was last zeroed) the cumulative books of every gate and the time go into row
 *            (substeps / stride - 1) mod history of a ring on the device: a long sph_dispatch_n or a replayed graph leaves a hydrograph.
 * The step writes no particle state.  The table, the count, history and stride live in device memory: a replayed graph sees a later
 * sph_gates_set; whether the step runs, and its buffers, enter a graph's key only while gates are set.  A set call with another count,
 * history or stride zeroes books and ring, one with the same three keeps them.  sph_reset drops the gates, sph_destroy frees them.
 * SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (no sorted copy); setting that option while gates exist makes the next dispatch
 * fail and change nothing.  SPH_ERR_ARG (the previous state stays): a count above SPH_MAX_GATES, a null table with count > 0, an unknown
 * shape or flag, a non-finite field, u or v of zero length, |u.v| > 1e-4 |u| |v| (in double), history above 4096, stride 0. */
#define SPH_MAX_GATES 8
#define SPH_MAX_GATE_HISTORY 4096
enum { SPH_GATE_RECT = 0, SPH_GATE_ELLIPSE = 1 };
enum { SPH_GATE_UNBOUNDED = 1 };
typedef struct SphGate {   /* 64 bytes */
    int32_t  shape;        /* SPH_GATE_RECT | SPH_GATE_ELLIPSE */
    int32_t  flags;        /* SPH_GATE_UNBOUNDED */
    float    center[3];
    float    u[3];         /* half-extent vectors; forward is cross(u, v) */
    float    v[3];
    float    pad[5];
} SphGate;
typedef struct SphGateBooks {   /* 72 bytes */
    uint64_t forward, backward;
    double   vel[3];
    double   scalar[4];    /* SPH_MAX_SCALAR_CHANNELS */
} SphGateBooks;
/* Replaces the gate table; count 0 clears it.  history: rows of the ring (0: none); stride >= 1.  Stream-ordered. */
int  sph_gates_set(SphEngine* e, const SphGate* gates, int count, uint32_t history, uint32_t stride);
/* The gates as set (cap >= count, else SPH_ERR_CAPACITY); any output pointer may be null. */
int  sph_gates_get(SphEngine* e, SphGate* out, int cap, int* countOut, uint32_t* historyOut, uint32_t* strideOut);
/* The books of the `count` gates, the simulated time and the substeps summed since the last zeroing; reset != 0 zeroes these (not the
 * ring) after the read.  Any output pointer may be null.  Synchronises. */
int  sph_gates_books(SphEngine* e, SphGateBooks* books, double* timeOut, uint64_t* substepsOut, int reset);
/* The stored ring rows in chronological order: *countOut <= history rows of `count` books each (rows: room for history * count records)
 * with their times (room for history), and the index of the first one (row i was taken after (first + i + 1) * stride substeps).
 * Any output pointer may be null.  Synchronises. */
int  sph_gates_history(SphEngine* e, uint64_t* firstOut, uint32_t* countOut, SphGateBooks* rows, double* times);
/* Host-only, no device: the same __host__ __device__ functions the kernel runs on n records at the entry and at the exit of one substep
 * (record i of both is the same particle), in index order, the sums added in index order INTO books[0 .. count-1].  values: n * channels
 * floats (record i owns values[i * channels ..]) or NULL with channels 0. */
int  sph_gates_step_host(const SphParticle* entry, const SphParticle* exitRecords, size_t n, const SphGate* gates, int count,
                         const float* values, int channels, SphGateBooks* books);

/* ---- field monitors: probes and lattices averaged inside the substep (no reference counterpart) -------------
 * A monitor is a fixed set of M points (1 <= M <= SPH_MAX_MONITOR_POINTS): m explicit (x, y, z, unused) rows, or the lattice
 * origin + (float)i * spacing, x fastest, the point formula of sph_sample_lattice.  Up to SPH_MAX_MONITORS independent monitors per
 * engine, addressed by `slot`.  Off by default; with no monitor set a dispatch launches exactly what it launched before.
 *   which substeps act   c = the non-paused substeps this monitor has seen since it was set or reset (a counter in device memory).  The
 *            substep acts iff c % every == 0: the first substep after a set acts and sees the state at set time.  With a = the acting
 *            substeps before this one, it also writes ring row (a / stride) % history iff history > 0 && a % stride == 0.
 *   what it samples      for each point the SphSample sph_sample_points would return on the state the substep STARTS from, evaluated on
 *            the sorted copy the substep has just built (where the tracers are advected): the sampler's own candidate function in the
 *            sampler's order, so a monitor sample is, bit for bit, sph_sample_points called just before the dispatch.
 *   accumulation         each point owns one SphMonitorRow; no atomics.  wet: fraction >= wetFraction.  Every update is
 *            sum = sum + (double)x or sum = sum + (double)a * (double)b (the product of two fp32 values is exact in fp64: fused or not,
 *            the same bits).  A sample with a non-finite field is skipped whole (the row's `samples` then stays below the monitor's
 *            `acting`); a non-finite POINT gives the sampler's all-zero record and counts as a dry sample.
 *   ring                 a ring row holds the raw SphSample of the points 0 .. ringPoints-1 and the fp64 time of the entry state (the
 *            sum of dt of the substeps before this one since set or reset).  history * ringPoints * 32 bytes <= 256 MiB.
 * every, stride, the ring geometry, the counters, wetFraction and a lattice's origin and spacing live in device memory: a replayed
 * graph sees a later set or reset.  A graph's key holds, only while a monitor is set, each slot's kind, M, a lattice's dims, the
 * buffers and the ring layout: sph_monitor_reset, and a set call that keeps these, need no new capture.  A set call on a slot always
 * restarts that slot (rows, counters, ring); sph_reset drops every monitor, param_pause leaves everything untouched.
 * SPH_ERR_STATE, before any allocation: z-slab engines and SPH_OPT_GRID_BUILD 1 (no sorted copy); setting that option while a monitor
 * exists makes the next dispatch fail and change nothing.  SPH_ERR_ARG (the previous state stays): slot out of range, null data with
 * m > 0, m above the cap, a lattice dim < 1 or a point count above the cap, a spacing not finite and > 0, an origin not finite,
 * every or stride of 0, history above SPH_MAX_MONITOR_HISTORY, ringPoints > M, a ring above 256 MiB, a wetFraction that is not finite.
 * SPH_ERR_CAPACITY from the download calls when the capacity is too small. */
#define SPH_MAX_MONITORS 4
#define SPH_MAX_MONITOR_POINTS 4194304
#define SPH_MAX_MONITOR_HISTORY 4096
enum { SPH_MONITOR_NONE = 0, SPH_MONITOR_POINTS = 1, SPH_MONITOR_LATTICE = 2 };   /* SphMonitorInfo.kind */
enum { SPH_MONITOR_WET_SHARE = 0, SPH_MONITOR_MEAN_FRACTION = 1, SPH_MONITOR_VAR_FRACTION = 2, SPH_MONITOR_MEAN_DENSITY = 3,
       SPH_MONITOR_MEAN_PRESSURE = 4, SPH_MONITOR_VAR_PRESSURE = 5, SPH_MONITOR_MEAN_VEL_X = 6, SPH_MONITOR_MEAN_VEL_Y = 7,
       SPH_MONITOR_MEAN_VEL_Z = 8, SPH_MONITOR_TKE = 9 };
typedef struct SphMonitorConfig {   /* 24 bytes */
    uint32_t every;        /* >= 1: every `every`-th non-paused substep acts */
    float    wetFraction;  /* a sample is wet iff fraction >= wetFraction (0.5) */
    uint32_t history;      /* ring rows, 0 .. SPH_MAX_MONITOR_HISTORY (0: no ring) */
    uint32_t stride;       /* >= 1: every `stride`-th acting substep writes a ring row */
    uint32_t ringPoints;   /* the ring keeps the points 0 .. ringPoints-1 (0 .. M; 0 with a history: min(M, 64)) */
    uint32_t pad;
} SphMonitorConfig;
typedef struct SphMonitorRow {        /* 128 bytes */
    uint64_t samples, wet;
    double sumFraction, sumFraction2, sumDensity;          /* over all samples            */
    double sumPressure, sumPressure2;                      /* over wet samples            */
    double sumVel[3];                                      /* over wet samples            */
    double sumVelVel[6];                                   /* xx, yy, zz, xy, xz, yz; wet */
} SphMonitorRow;
typedef struct SphMonitorInfo {   /* 112 bytes */
    int32_t  kind;         /* SPH_MONITOR_NONE (an empty slot: everything else 0) | _POINTS | _LATTICE */
    int32_t  dims[3];      /* lattice: nx, ny, nz; points: M, 1, 1 */
    uint64_t points;       /* M */
    SphMonitorConfig config;   /* as set, ringPoints as in force */
    uint64_t substeps;     /* c: non-paused substeps seen since set / reset */
    uint64_t acting;       /* a: those of them that acted */
    double   time;         /* sum of dt over the c substeps */
    uint64_t firstRow;     /* index of the oldest ring row held (ring row r was written by acting substep r * stride) */
    uint32_t ringRows;     /* ring rows held, <= history */
    uint32_t pad;
    float    origin[3], spacing[3];   /* lattice */
} SphMonitorInfo;
void sph_monitor_config_default(SphMonitorConfig* out);   /* every 1, wetFraction 0.5, history 0, stride 1, ringPoints 0 */
/* Sets slot `slot` to m explicit points (4 floats each, host / device memory); config NULL: the defaults; m 0 clears the slot.  The
 * points are copied. */
int  sph_monitor_set(SphEngine* e, int slot, const float* points4, size_t m, const SphMonitorConfig* config);
int  sph_monitor_set_device(SphEngine* e, int slot, const float* devPoints4, size_t m, const SphMonitorConfig* config);
/* Sets slot `slot` to the lattice of dims[0] x dims[1] x dims[2] points; row index (l * ny + j) * nx + i. */
int  sph_monitor_set_lattice(SphEngine* e, int slot, const float origin[3], const float spacing[3], const int dims[3], const SphMonitorConfig* config);
/* What slot `slot` holds, with the device's counters.  Synchronises. */
int  sph_monitor_info(SphEngine* e, int slot, SphMonitorInfo* out);
/* The M rows in the caller's order (cap >= M rows, else SPH_ERR_CAPACITY).  Synchronises. */
int  sph_monitor_download(SphEngine* e, int slot, SphMonitorRow* out, size_t cap);
/* Borrowed device address of the rows (NULL for an empty slot); valid until the slot is set, cleared or the engine reset.  No synchronisation. */
int  sph_monitor_device(SphEngine* e, int slot, const SphMonitorRow** devPtr);
/* The ring rows held, oldest first: *countOut rows of ringPoints samples each (row k, point p at samples[k * ringPoints + p]) with
 * their times and the index of the first (rowCap >= rows held, else SPH_ERR_CAPACITY).  Any output pointer may be null.  Synchronises. */
int  sph_monitor_history(SphEngine* e, int slot, uint64_t* firstOut, uint32_t* countOut, SphSample* samples, double* times, size_t rowCap);
/* A derived volume: M floats into device memory.  Every operation in fp64 and rounded on its own, then one rounding to fp32; 0 where
 * the dividing count is 0:  WET_SHARE wet / samples; MEAN_FRACTION sumFraction / samples; VAR_FRACTION sumFraction2 / samples - mean^2;
 * MEAN_DENSITY sumDensity / samples; MEAN_PRESSURE sumPressure / wet; VAR_PRESSURE sumPressure2 / wet - mean^2; MEAN_VEL_a sumVel[a] / wet;
 * TKE 0.5 * (((xx / wet - mx^2) + (yy / wet - my^2)) + (zz / wet - mz^2)).  SPH_ERR_STATE on an empty slot.  Stream-ordered. */
int  sph_monitor_field(SphEngine* e, int slot, int field, float* devOut);
/* Zeroes rows, counters and ring on the stream and keeps the buffers (averaging can begin after a spin-up; a captured graph stays valid). */
int  sph_monitor_reset(SphEngine* e, int slot);
/* Drops slot `slot` and frees its buffers; slot < 0: every slot. */
int  sph_monitor_clear(SphEngine* e, int slot);
/* Host-only, no device, plain loops over the same __host__ __device__ functions the kernels run: one acting substep of m samples INTO
 * rows[0 .. m), and a derived field of m rows. */
int  sph_monitor_accumulate_host(SphMonitorRow* rows, const SphSample* samples, size_t m, float wetFraction);
int  sph_monitor_field_host(const SphMonitorRow* rows, size_t m, int field, float* out);
/* Host-only: the counters' rule over `substeps` substeps after a set: actsOut[s] = 1 iff substep s acts, rowsOut[s] = the ring row it
 * writes or 0xFFFFFFFF (what k_monitor_tick runs). */
int  sph_monitor_schedule_host(uint32_t every, uint32_t stride, uint32_t history, size_t substeps, uint32_t* actsOut, uint32_t* rowsOut);

/* ---- spray, foam and bubbles: secondary particles spawned by the fluid (no reference counterpart) -----------
 * Secondary ("diffuse") particles in the sense of Ihmsen et al. 2012, reduced to what the engine's state supports: points that do not
 * act on the fluid, born where the fluid foams (padA, the foam factor every substep computes), classed every substep by how much fluid
 * surrounds them, moved by class, aged and removed.  Off by default; with no pool set a dispatch launches exactly what it launched before.
 * The pool is a SEQUENCE of at most `capacity` records.  One substep, on the state the substep STARTS from (behind the grid build, in
 * front of the SPH pass and of the fountain / river recycle), with u = vel and n = count of the SphSample that sph_sample_points gives at
 * the record's position, g the params' gravity, every fp32 expression a multiply and then an add (no fma), in the order written:
 *   1. advance  n < sprayBelow: spray   v' = v + dt g;                                  x' = x + dt v'
 *               n > bubbleAbove: bubble v' = (v - (dt kb) g) + kd (u - v);              x' = x + dt v'
 *               otherwise: foam         v' = u;  x' = x + dt u;  life' = life - dt
 *               age' = age + dt for every class; kind = the class.  The record dies, counted under the FIRST cause that holds, if a
 *               coordinate of x' is not finite, x' lies outside the grid's box [gridMin, gridMin + (float)dims * cellSize] (bounds
 *               included), not life' > 0, age' > maxAge.
 *   2. spawn    a fluid particle (isGhost == 0; isActive says something about ghosts only, the spawners write 0) with density > 0 (read as
 *               the sorted copy's 1/rho > 0) and a finite padA > threshold has min(floor((rate dt) (padA - threshold) + U_0), maxPerParent)
 *               children; child k is born at pos + (spread h) (2 U - 1) per axis (U_{1+4k}, U_{2+4k}, U_{3+4k}) with the parent's velocity,
 *               life = lifeMin + U_{4+4k} (lifeMax - lifeMin), age 0, parent = the particle's id, birth = the low word of the substep
 *               counter, kind = SPH_DIFFUSE_FOAM until its first substep classes it.  U_d = (hash >> 8) 2^-24 with hash =
 *               mix(mix(mix(mix(mix(seed + 0x9e3779b9) ^ id) ^ counterLow) ^ counterHigh) ^ d), mix(x): x ^= x >> 16; x *= 0x7feb352d;
 *               x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 -- no state is carried.
 *   3. order    the survivors keep their relative order; the newborn follow in (parent id ascending, k ascending); newborn that would
 *               exceed the capacity are dropped from the END of that order and counted.
 *   4. the 64-bit substep counter and the running totals advance (device memory).
 * Hence the pool after n substeps equals, bit for bit and order included, the host loop
 *   s = sph_sample_points(pool positions); P = sph_download_particles; sph_dispatch(dt); pool = sph_diffuse_step_host(pool, s, P, ...)
 * also through sph_dispatch_n and captured graphs, and the particle records are byte-identical with and without a pool.
 * param_pause: nothing happens.  Impulses, uploads and sph_set_params do not touch the pool; sph_reset drops it.  Timed as SPH_K_OTHER.
 * SPH_ERR_STATE from sph_diffuse_set, before anything is allocated, on z-slab engines and under SPH_OPT_GRID_BUILD 1; setting
 * SPH_OPT_GRID_BUILD 1 while a pool exists makes the next dispatch fail with SPH_ERR_STATE and change nothing.  SPH_ERR_ARG (the previous
 * config stays in force): a rate, lifeMin, lifeMax or spread that is not finite or negative, lifeMax < lifeMin, maxPerParent outside
 * 1 .. 8, sprayBelow > bubbleAbove, kd outside [0, 1], a threshold or kb that is not finite, a maxAge that is NaN or negative, a capacity
 * above 2^31 - 1. */
typedef struct SphDiffuse { float pos[3]; float life; float vel[3]; float age; uint32_t parent; uint32_t birth; uint32_t kind; uint32_t pad; } SphDiffuse;   /* 48 bytes */
enum { SPH_DIFFUSE_SPRAY = 0, SPH_DIFFUSE_FOAM = 1, SPH_DIFFUSE_BUBBLE = 2 };
typedef struct SphDiffuseConfig {
    uint32_t capacity;       /* C: records the pool can hold (0: no pool) */
    uint32_t seed;           /* of the hash */
    float    threshold;      /* padA above which a particle spawns */
    float    rate;           /* children per second and unit of padA above the threshold */
    float    lifeMin, lifeMax;   /* seconds; only foam loses life */
    float    spread;         /* half width of the birth cube in units of h */
    float    maxAge;         /* seconds; bounds every class */
    uint32_t sprayBelow;     /* n below this: spray */
    uint32_t bubbleAbove;    /* n above this: bubble */
    float    kb;             /* buoyancy of a bubble in units of gravity */
    float    kd;             /* drag of a bubble towards the fluid's velocity per substep, 0 .. 1 */
    uint32_t maxPerParent;   /* 1 .. 8 */
    uint32_t pad[3];
} SphDiffuseConfig;          /* 64 bytes */
typedef struct SphDiffuseInfo {
    uint64_t substeps;       /* the device counter: substeps that stepped this pool */
    uint64_t spawned, dropped, diedLife, diedAge, leftBox, nonFinite;   /* running totals since the pool was made */
    uint64_t seeded;         /* records sph_diffuse_seed put in: alive == seeded + spawned - dropped - the four deaths */
    uint32_t alive, capacity;
    uint32_t aliveByKind[3]; /* by the records' kind after the last substep */
    uint32_t pad;
} SphDiffuseInfo;            /* 88 bytes */
/* The defaults DESIGN.md section 3j argues for (capacity 65536). */
void sph_diffuse_default(SphDiffuseConfig* out);
/* NULL or capacity 0 drops the pool.  The capacity of the pool in place: the pool stays and the coefficients are replaced (stream-ordered,
 * no re-capture of a graph); another capacity: a new, empty pool with counters at zero. */
int  sph_diffuse_set(SphEngine* e, const SphDiffuseConfig* cfg);
/* The config in force (capacity 0 without a pool). */
int  sph_diffuse_get(SphEngine* e, SphDiffuseConfig* out);
/* Counter, alive count and totals (zeros without a pool).  Synchronises. */
int  sph_diffuse_info(SphEngine* e, SphDiffuseInfo* out);
/* The living records in pool order to HOST memory (cap >= alive, else SPH_ERR_CAPACITY, nothing written).  Synchronises. */
int  sph_diffuse_download(SphEngine* e, SphDiffuse* out, size_t cap, size_t* countOut);
/* Borrowed device addresses of the records and of the word that holds the alive count (null without a pool); valid until the pool is
 * dropped or re-made.  A kernel of the host's on the engine's stream sees the pool after the last enqueued substep. */
int  sph_diffuse_device(SphEngine* e, const SphDiffuse** records, const uint32_t** aliveCountWord);
/* m caller-made records behind the living ones, for tests and for emitters of the host's own (alive + m <= capacity, else
 * SPH_ERR_CAPACITY, nothing written; SPH_ERR_STATE without a pool).  The records are taken as they are.  Synchronises. */
int  sph_diffuse_seed(SphEngine* e, const SphDiffuse* records, size_t m);
/* Host-only, no device: the same __host__ __device__ functions the kernels run, in plain loops.  pool[0 .. m) with samples[i] the SphSample
 * at pool[i].pos, particles[0 .. n) the state the substep starts from (id = index), substep = the counter before the step; out needs room
 * for cfg->capacity records.  totals (may be null) is advanced like the device's, `substeps` included.  dt <= 0: param_timeStep.
 * param_pause: out = pool. */
int  sph_diffuse_step_host(const SphDiffuseConfig* cfg, const SphParams* params, float dt, uint64_t substep, const SphDiffuse* pool, size_t m,
                           const SphSample* samples, const SphParticle* particles, size_t n, SphDiffuse* out, size_t* countOut, SphDiffuseInfo* totals);

/* ---- births at wave crests: a second, optional birth term of the pool ("crest births") ---------------------
 * Ihmsen et al.'s wave-crest potential, from the free-surface rows of section 3o: a fluid particle of the shell whose surface is sharply
 * convex (crest) and which moves along its own outward normal bears children, wherever padA stands.  Off by default; with the term off a
 * substep launches what it launched before and the pool, the records and the graph keys are the same bytes.  The config belongs to the
 * pool.  Everything is fp32, every operation rounded on its own (no fma but those of shell_add), dot3 as elsewhere, sqrtf and / correctly
 * rounded, in the order written:
 *   acting   a substep ACTS when the pool's 64-bit substep counter before the step is a multiple of `every`; on other substeps the term
 *            bears nobody (its kernels are launched and return at once: a captured graph has a fixed launch list).
 *   shell    on an acting substep the SphShell rows (normal, crest, flags) of sph_shell_build with (radius, offset, minCount, flags) on the
 *            substep's ENTRY state: the same neighbor_offset / shell_add / shell_finish / shell_crest_term / shell_crest_value over the sorted
 *            copy the substep has just built, whose slot order is HostGrid's (cell, id) order; hence the bytes of sph_shell_host.
 *   who      a particle QUALIFIES when isGhost == 0, the sorted copy's 1/rho > 0, its row has SPH_SHELL_MEMBER and not
 *            SPH_SHELL_ISOLATED, sp2 = dot3(v, v) is finite, sp = sqrtf(sp2) > 0 and dot3(v, normal) >= align * sp.
 *   how many pc = fminf(fmaxf((crest - crestMin) / (crestMax - crestMin), 0), 1); pk = fminf(fmaxf((sp - speedMin) / (speedMax - speedMin), 0), 1);
 *            p = pc * pk; nobody where not p > 0; lam = ((rate * dt) * (float)every) * p; c = floorf(lam + U_33), taken as maxPerParent
 *            where not c < (float)maxPerParent (U_33: draw 33 of the hash above, the first draw the eight children of a parent do not use).
 *            With f the children of the foam term (step 2 above, exactly as it is, draw 0 included) the parent has min(f + c, maxPerParent)
 *            children: k = 0 .. f - 1 are the foam term's, the crest term's follow them.  Placement, life, order, dropping from the end
 *            and the books' identity are those of steps 2 to 4; crest children are counted in `spawned` too.
 *   books    SphDiffuseCrestInfo: acting substeps, crest children before dropping, the number of shell members of the last acting substep
 *            (device memory, no atomics: per-block rows added up behind the count).  They live as long as the pool.
 * Hence the pool and the books equal, bit for bit and order included, the host loop of the block above with
 *   rows = sph_shell_host(P, (radius, offset, minCount, flags)) (or sph_shell_build + download, the same bytes) in front of the dispatch
 * and sph_diffuse_step_host_crest in place of sph_diffuse_step_host, also through sph_dispatch_n and captured graphs.  rate, the two
 * windows, align and every are read from device memory: a replayed graph sees a change without a new capture; radius, offset, minCount
 * and flags are launch arguments (a change captures anew).
 * sph_diffuse_set with the capacity in place keeps the crest config; another capacity, NULL, sph_reset and sph_destroy drop it.
 * SPH_ERR_STATE from sph_diffuse_set_crest without a pool (and the pool's own refusals hold); SPH_ERR_STATE from a dispatch whose grid
 * makes the radius exceed three cells.  SPH_ERR_ARG (the previous state stays in force): a rate that is not finite or negative, a radius
 * that is not finite or above three cells of the current params' grid, an offset that is not finite or negative, a window that is empty
 * (min >= max) or not finite, align outside [0, 1], every == 0, unknown flag bits. */
typedef struct SphDiffuseCrest {
    float    rate;           /* children per second at full potential (pc = pk = 1); 0: the term is off */
    float    radius;         /* of the shell pass; <= 0: param_h; at most three cells (SphShellConfig's rule) */
    float    offset;         /* SphShellConfig.offset */
    uint32_t minCount;       /* SphShellConfig.minCount */
    int32_t  flags;          /* SphShellConfig.flags (SPH_SHELL_FLUID_ONLY) */
    float    crestMin, crestMax;   /* the clamp window of the crest sum, crestMin < crestMax */
    float    speedMin, speedMax;   /* the clamp window of the speed, speedMin < speedMax */
    float    align;          /* 0 .. 1: the cosine between velocity and normal a parent needs at least (the paper's 0.6) */
    uint32_t every;          /* >= 1: the term acts on substeps whose counter is a multiple of it */
    uint32_t pad;
} SphDiffuseCrest;           /* 48 bytes */
typedef struct SphDiffuseCrestInfo {
    uint64_t acting;         /* substeps on which the term acted */
    uint64_t crestSpawned;   /* children of the crest term before dropping (part of SphDiffuseInfo.spawned) */
    uint32_t shellSize;      /* shell members of the last acting substep */
    int32_t  on;             /* 1 while the term is switched on */
    float    radius;         /* the radius in force at the current params (0 while off) */
    int32_t  stencil;        /* its half-width in cells (0 while off) */
} SphDiffuseCrestInfo;       /* 32 bytes */
/* The defaults DESIGN.md section 3j argues for (a starting point, chosen on the default scene). */
void sph_diffuse_crest_default(SphDiffuseCrest* out);
/* NULL or rate == 0 switches the term off (the books stay).  Stream-ordered; no re-capture of a graph unless a launch argument changes. */
int  sph_diffuse_set_crest(SphEngine* e, const SphDiffuseCrest* crest);
/* The config in force (all zero while off or without a pool). */
int  sph_diffuse_get_crest(SphEngine* e, SphDiffuseCrest* out);
/* The books (zeros without a pool).  Synchronises. */
int  sph_diffuse_crest_info(SphEngine* e, SphDiffuseCrestInfo* out);
/* sph_diffuse_step_host with the crest term: crest (NULL or rate == 0: exactly sph_diffuse_step_host) and shellRows[0 .. n), the SphShell
 * rows by id of the state the substep starts from (sph_shell_host or sph_shell_build with the crest config's radius, offset, minCount and
 * flags; needed when crest is on and n > 0).  crestTotals (may be null) is advanced like the device's books. */
struct SphShell;             /* (defined with the free-surface particles below) */
int  sph_diffuse_step_host_crest(const SphDiffuseConfig* cfg, const SphDiffuseCrest* crest, const SphParams* params, float dt, uint64_t substep,
                                 const SphDiffuse* pool, size_t m, const SphSample* samples, const SphParticle* particles, size_t n,
                                 const struct SphShell* shellRows, SphDiffuse* out, size_t* countOut, SphDiffuseInfo* totals,
                                 SphDiffuseCrestInfo* crestTotals);

/* ---- fixed-radius neighbour lists in CSR form (no reference counterpart) --------------------------------------
 * The engine's neighbour relation as an output: for every particle, or for arbitrary query points, the particles within a radius R,
 * on the device, in the engine's fixed order.  The grid is that of the CURRENT state, built exactly as sph_sample_points builds it
 * (cells from BuildGrid's formula: (x - gridMin) / cellSize with IEEE division, floorf, clamp).  For 0 < R <= 3 * cellSize:
 *   R2 = R * R in fp32; the stencil half-width s is the smallest of 1, 2, 3 with R <= (float)s * cellSize;
 *   the candidates of a target in cell (cx, cy, cz) are the members of the cells [c - s, c + s] per axis that lie inside the grid;
 *   candidate j is accepted when r2 < R2, r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with d = x_target - x_j (at R = h: sweep 1's test
 *   and the `count` of SphSample);
 *   the accepted candidates stand in ascending sorted slot, i.e. ascending (cell index, particle id) -- for s = 1 the order the SPH
 *   pass visits them; entries are particle ids (the index into the 80-byte array) as int32; rows are numbered by particle id
 *   (particle lists) or by query point (query lists); offsets is int64[rows + 1] and offsets[rows] the total.
 * Particle lists: the target's own slot is left out by default; SPH_NEIGHBORS_SELF keeps it (by slot identity, not by distance);
 * SPH_NEIGHBORS_HALF keeps only id_j > id_i (an undirected edge list); SELF | HALF is SPH_ERR_ARG.  Every record has a row, ghosts and
 * inactive records included.  Query lists: SELF and HALF are SPH_ERR_ARG; a point with a non-finite coordinate has an empty row.  A
 * particle with a non-finite position is accepted by nobody (r2 is NaN).  SPH_NEIGHBORS_COUNT_ONLY builds offsets and maxCount only.
 * Bit for bit: the relation is symmetric (j in N(i) <=> i in N(j)), and at R = h with SELF the length of row i equals the `count` of
 * sph_sample_points at particle i's position.
 * The lists are engine-owned and stay valid until the next sph_neighbors_build / _query, sph_reset or sph_destroy; a dispatch does not
 * touch them (they describe the state they were built from) and a build never changes the simulation.  maxPairs > 0 and a total above
 * it: SPH_ERR_CAPACITY after the count pass, *out filled, offsets valid, no index buffer.  Timed as SPH_K_OTHER (the grid build under
 * bin / scan / scatter).  SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1, as sampling.  SPH_ERR_ARG: a null argument, an R that
 * is not finite, <= 0 or above 3 * cellSize, unknown flag bits, more than 2^31 - 1 query points. */
enum { SPH_NEIGHBORS_SELF = 1, SPH_NEIGHBORS_HALF = 2, SPH_NEIGHBORS_COUNT_ONLY = 4 };
typedef struct SphNeighborInfo { uint64_t rows, total; float radius; int32_t stencil, flags, kind /*0 none, 1 particles, 2 query*/; uint32_t maxCount, pad; } SphNeighborInfo;   /* 40 bytes */
/* Lists of every particle.  Synchronises. */
int sph_neighbors_build(SphEngine* e, float radius, int flags, uint64_t maxPairs, SphNeighborInfo* out);
/* Lists of m query points of 4 floats (x, y, z, unused) in DEVICE memory.  Synchronises. */
int sph_neighbors_query(SphEngine* e, const float* devPoints4, size_t m, float radius, int flags, uint64_t maxPairs, SphNeighborInfo* out);
/* What the engine holds (kind 0 before any build). */
int sph_neighbors_info(const SphEngine* e, SphNeighborInfo* out);
/* Borrowed device addresses: offsets[rows + 1], indices[total] (null for count-only or refused lists).  SPH_ERR_STATE without lists. */
int sph_neighbors_device(SphEngine* e, const int64_t** offsets, const int32_t** indices);
/* Device-to-device copies into the caller's memory on the engine's stream (asynchronous), and copies to HOST memory (synchronises).
 * SPH_ERR_STATE without lists; SPH_ERR_CAPACITY (nothing written) if indexCap is below the total; SPH_ERR_ARG for a null offsets, or a
 * null indices while the engine holds at least one (count-only, refused and empty lists hold none: indices is then ignored). */
int sph_neighbors_export(SphEngine* e, int64_t* devOffsets, int32_t* devIndices, uint64_t indexCap);
int sph_neighbors_download(SphEngine* e, int64_t* offsets, int32_t* indices, uint64_t indexCap);
/* Host-only, no device: the same neighbor_accept over a counting sort of its own (cells ascending, members ascending by index).
 * points4 NULL: particle lists of particles[0 .. n) (m ignored); else query lists of m points.  offsets needs rows + 1 entries;
 * a total above indexCap: SPH_ERR_CAPACITY with *out filled and offsets valid (so a COUNT_ONLY call sizes the second one). */
int sph_neighbors_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m,
                       float radius, int flags, int64_t* offsets, int32_t* indices, uint64_t indexCap, SphNeighborInfo* out);

/* ---- connected components: which particles hang together (no reference counterpart) --------------------------
 * The graph of the neighbour relation above (same grid of the CURRENT state, radius rules 0 < R <= 3 * cellSize, stencil half-width and
 * accept test): records i != j are joined when j is a candidate of i and r2 < R2.  A component is a connected component of that graph;
 * every participating record is in exactly one, a record with no edge is a component of one.  A record with a non-finite coordinate is
 * accepted by nobody: a component of one with SPH_COMPONENT_NONFINITE in its row's flags.  By default every record takes part;
 * SPH_COMPONENTS_FLUID_ONLY leaves out the records with isGhost != 0: they join nothing, bridge nothing, and get label and root -1.
 *   roots[i]  = the smallest particle id in i's component; components are numbered 0 .. C-1 in ascending order of that id and
 *   labels[i] = that number; both int32[n], indexed by particle id.  Row c of the table describes component c: its root, the number of
 *   members, the fp32 minimum and maximum of their positions, and sumQ, the sum over the members of the fixed-point position
 *   q = llrint(clamp(((double)x - (double)gridMin) * S, -2^36, 2^36)) per axis, S = 65536.0 / (double)cellSize (subtract, then multiply,
 *   each rounded in fp64; round to nearest even).  The centre of a body is gridMin + cellSize * sumQ / (65536 * count).  A non-finite
 *   component has a zero box and zero sums.  Everything is integer from the accept test on: the same bytes on every run.
 * The buffers are engine-owned and stay valid until the next sph_components_build, sph_reset or sph_destroy; a dispatch does not touch
 * them and a build never changes the simulation.  Timed as SPH_K_OTHER.  SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as
 * sampling); _info / _device / _download before any build; a build that needed more than 64 rounds (no result is left).  SPH_ERR_ARG: a
 * null argument, a bad R, unknown flag bits.  n = 0: everything zero or empty, the call succeeds. */
enum { SPH_COMPONENTS_FLUID_ONLY = 1 };
enum { SPH_COMPONENT_NONFINITE = 1 };
typedef struct SphComponent { uint32_t root, count; float bbMin[3], bbMax[3]; int64_t sumQ[3]; uint32_t flags, pad; } SphComponent;   /* 64 bytes */
typedef struct SphComponentInfo {
    uint64_t rows, numComponents, numExcluded, largestCount;
    uint32_t largestRoot /* ties go to the smaller root */, numSingletons;
    float radius;
    int32_t stencil, flags;
    uint32_t rounds /* hook launches used (0 from sph_components_host) */;
} SphComponentInfo;   /* 56 bytes */
/* Labels, roots and table of the current state.  Synchronises. */
int sph_components_build(SphEngine* e, float radius, int flags, SphComponentInfo* out);
int sph_components_info(const SphEngine* e, SphComponentInfo* out);
/* Borrowed device addresses: labels[rows], roots[rows], table[numComponents]. */
int sph_components_device(SphEngine* e, const int32_t** labels, const int32_t** roots, const SphComponent** table);
/* Copies into the caller's memory, host or device (the kind of each copy follows from the address); synchronises; any pointer may be
 * null.  SPH_ERR_CAPACITY (nothing written) if table is given and tableCap is
 * below numComponents. */
int sph_components_download(SphEngine* e, int32_t* labels, int32_t* roots, SphComponent* table, uint64_t tableCap);
/* Host-only, no device: a sequential union-find over the counting sort of sph_neighbors_host with the same accept function; the same
 * bytes (rounds = 0).  labels, roots and table may be null; *out is filled before a tableCap refusal (nothing else is written then). */
int sph_components_host(const SphParticle* particles, size_t n, const SphParams* params, float radius, int flags,
                        int32_t* labels, int32_t* roots, SphComponent* table, uint64_t tableCap, SphComponentInfo* out);

/* ---- k nearest neighbours within a radius (no reference counterpart) ------------------------------------------
 * For every particle, or for arbitrary query points, the k nearest particles within a radius R, nearest first, on the device.  Grid
 * (of the CURRENT state), radius rules 0 < R <= 3 * cellSize, R2 = R * R in fp32, stencil half-width and candidates are those of the
 * neighbour lists above.  Candidate j is accepted when r2 < R2 with the same r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), d = x_target -
 * x_j, and has the key ((uint64)bits(r2) << 32) | id_j: r2 is >= +0, so keys compared as uint64 order by ascending r2 and, among equal
 * r2, by ascending particle id.  The row of a target is its min(k, accepted) smallest keys, ascending -- one answer whatever the order
 * in which candidates are met, also on lattices and for coincident particles, and the same bytes on every run.  1 <= k <= SPH_KNN_MAX_K.
 * Particle rows are numbered by particle id and every record has a row; the target's own slot is left out by slot identity.
 * NOTE, SPH_KNN_SELF is not SPH_NEIGHBORS_SELF: with it the own slot is an ORDINARY candidate (r2 = 0, placed by id among coincident
 * particles), so a target with a non-finite position still has an empty row (the neighbour lists keep such a target by identity).
 * SPH_KNN_FLUID_ONLY: records with isGhost != 0 are never candidates and their own rows are empty.  Query rows are numbered by query
 * point: SELF is SPH_ERR_ARG, FLUID_ONLY is allowed, a point with a non-finite coordinate has an empty row.
 * Outputs, engine-owned, dense and row-major: indices int32[rows * k] (particle ids, padded with -1), dist2 float[rows * k] (the fp32 r2
 * of each entry bit for bit, padded with +inf), counts uint32[rows].  SphKnnInfo: total = the sum of the counts, rowsFull = the rows with
 * count == k (integer reductions).  Bit for bit: the row for k1 is a prefix of the row for k2 > k1; counts[i] = min(k, degree_i) with the
 * degree of sph_neighbors_build at the same R (SELF for SELF), and for k >= degree_i the row holds exactly that list's ids; dist2
 * ascends along a row and equal dist2 have ascending ids.
 * The buffers stay valid until the next sph_knn_build / _query, sph_reset or sph_destroy; the neighbour lists and the components have
 * buffers of their own (neither kind of call invalidates the other); a dispatch does not touch them and a build never changes the
 * simulation.  Timed as SPH_K_OTHER.  SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as sampling); _info / _device / _download
 * before any build.  SPH_ERR_ARG: a null argument, a bad R, k outside 1 .. 64, unknown flag bits, more than 2^31 - 1 query points.
 * n = 0 or m = 0: empty results, the call succeeds. */
enum { SPH_KNN_SELF = 1, SPH_KNN_FLUID_ONLY = 2 };
enum { SPH_KNN_MAX_K = 64 };
typedef struct SphKnnInfo { uint64_t rows, total, rowsFull; float radius; int32_t k, stencil, flags, kind /*0 none, 1 particles, 2 query*/, pad; } SphKnnInfo;   /* 48 bytes */
/* Rows of every particle.  Synchronises. */
int sph_knn_build(SphEngine* e, int k, float radius, int flags, SphKnnInfo* out);
/* Rows of m query points of 4 floats (x, y, z, unused) in DEVICE memory (may be null when m is 0).  Synchronises. */
int sph_knn_query(SphEngine* e, const float* devPoints4, size_t m, int k, float radius, int flags, SphKnnInfo* out);
/* What the engine holds. */
int sph_knn_info(const SphEngine* e, SphKnnInfo* out);
/* Borrowed device addresses: indices[rows * k], dist2[rows * k], counts[rows]. */
int sph_knn_device(SphEngine* e, const int32_t** indices, const float** dist2, const uint32_t** counts);
/* Copies into the caller's memory, host or device (the kind of each copy follows from the address); synchronises; any pointer may be
 * null. */
int sph_knn_download(SphEngine* e, int32_t* indices, float* dist2, uint32_t* counts);
/* Host-only, no device: the counting sort of sph_neighbors_host and the same r2; per row the accepted keys are collected, sorted and
 * cut at k; the same bytes.  points4 NULL: particle rows of particles[0 .. n) (m ignored); else query rows of m points.  indices,
 * dist2 and counts may be null. */
int sph_knn_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m, int k, float radius, int flags,
                 int32_t* indices, float* dist2, uint32_t* counts, SphKnnInfo* out);

/* ---- ray casts against the particles (no reference counterpart) ----------------------------------------------
 * Every participating record is a solid sphere of radius r around its position; for each of m rays the call gives the first sphere the
 * ray ENTERS, on the device.  A ray is 8 floats, (ox, oy, oz, tmin), (dx, dy, dz, tmax); t is in units of the given direction (nothing
 * is normalised) and tmax = +inf is allowed.  A ray is void, and a miss, when any of o, d, tmin is not finite, tmax is NaN,
 * a = dot3(d, d) is 0 or not finite, or tmin > tmax.  0 < r <= 0.5f * cellSize (tested in fp32), r2 = r * r in fp32.
 * A record takes part when floorf((x - gridMin) / cellSize) lies in [0, dims) on every axis BEFORE the clamp of the grid build (records
 * outside the grid's box neither hit nor block; a NaN fails the compares); ghosts and inactive records take part like any other, and
 * SPH_RAYS_FLUID_ONLY leaves out records with isGhost != 0.
 * Per candidate, every operation rounded on its own except the fmaf()s: L = x_j - o, tca = dot3(L, d) * (1 / a), q = fmaf(-tca, d, L)
 * per axis, s = r2 - dot3(q, q); s < 0 is a miss; t = tca - sqrtf(s * (1 / a)) (IEEE division and square root on both sides); accepted
 * when tmin <= t <= tmax.  Only entries count: a sphere that contains the ray's start has t < tmin and is not hit.
 * key(j) = ((uint64)ordered(t) << 32) | id_j, ordered() the sign-flip map from float bits to unsigned order; the result of a ray is
 * the smallest key over all accepted participating records -- one answer whatever the order in which candidates are met, also on
 * lattices and for coincident particles, and the same bytes on every run.  The result does not name the grid.
 * Output: one SphRayHit per ray, in ray order: pos = fmaf(t, d, o) per axis, normal = (pos - x_id) * (1 / r); a miss is t = +inf,
 * id = -1, the rest 0.  SPH_RAYS_ANY_HIT: only whether anything is accepted -- id 0 and t 0 on a hit, id -1 and t +inf on a miss, the
 * rest 0; by definition it equals (first-hit id >= 0).  SphRaysInfo: hits and voidRays are integer reductions.
 * The hits stay valid until the next sph_rays_cast / _cast_device, sph_reset or sph_destroy; a cast changes no record, a dispatch does
 * not touch the hits, and neighbour lists, components and kNN rows have buffers of their own (no call of one kind invalidates
 * another's).  Timed as SPH_K_OTHER.  SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as sampling); _info / _device / _download
 * before any cast.  SPH_ERR_ARG: a null argument, a bad r, unknown flag bits, m > 2^31 - 1.  m = 0: no hits; n = 0: every ray a miss;
 * the call succeeds. */
enum { SPH_RAYS_FLUID_ONLY = 1, SPH_RAYS_ANY_HIT = 2 };
typedef struct SphRayHit { float t; int32_t id; float pos[3]; float normal[3]; } SphRayHit;   /* 32 bytes */
typedef struct SphRaysInfo { uint64_t rays, hits, voidRays; float radius; int32_t flags; } SphRaysInfo;   /* 32 bytes */
/* m rays of 8 floats in HOST memory (may be null when m is 0): staged upload, then as _cast_device.  Synchronises. */
int sph_rays_cast(SphEngine* e, const float* rays8, size_t m, float radius, int flags, SphRaysInfo* out);
/* m rays of 8 floats in DEVICE memory (may be null when m is 0).  One synchronisation, for the two counts. */
int sph_rays_cast_device(SphEngine* e, const float* devRays8, size_t m, float radius, int flags, SphRaysInfo* out);
/* What the engine holds. */
int sph_rays_info(const SphEngine* e, SphRaysInfo* out);
/* Borrowed device address: hits[rays]. */
int sph_rays_device(SphEngine* e, const SphRayHit** hits);
/* Copies the hits into the caller's memory, host or device (the kind of the copy follows from the address); synchronises. */
int sph_rays_download(SphEngine* e, SphRayHit* hits);
/* Host-only, no device, THE DEFINITION: brute force over all participating records, no grid, the same ray_hit; the same bytes.
 * hits may be null. */
int sph_rays_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                  SphRayHit* hits, SphRaysInfo* out);
/* TEST HOOK, not part of what an application needs.  Host-only, no device: the DEVICE's walk (the same ray_walk function) over the grid
 * as the counting sort leaves it.  Same bytes as sph_rays_host while the walk is complete; it is there so that the walk can be tested
 * against the definition without a device. */
int sph_rays_walk_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                       SphRayHit* hits, SphRaysInfo* out);

/* ---- ray spans: what each ray crosses in all (no reference counterpart; DESIGN.md section 3n "Spans") -------------------------------
 * The other half of a cast: how much of the fluid lies along the ray and where the ray leaves it.  Rays, void rays, the radius bound,
 * participation and SPH_RAYS_FLUID_ONLY are those of the cast; SPH_RAYS_ANY_HIT is SPH_ERR_ARG here.
 * With tca and thc = sqrtf(s * (1 / a)) exactly as above, tin = fmaxf(tca - thc, tmin), tout = fminf(tca + thc, tmax): a sphere is
 * CROSSED iff s >= 0 && tin < tout (a chord of positive length inside the window).  Unlike the cast, a sphere that contains the ray's
 * start counts, with tin = tmin.  Its share of a diameter is f = fminf((tout - tin) / (2 * thc), 1), q = (uint32)fmaf(f, 16777216, 0.5f).
 * Per ray one SphRaySpan: tEnter the smallest tin (+inf if nothing is crossed), tExit the largest tout (-inf), idEnter the id of the
 * smallest key (ordered(tin), id) (the cast's key rule; -1), idExit the id of the largest ordered(tout), ties to the smaller id (-1),
 * count the number of crossed spheres, flags bit 0 = the ray is void, length the sum of q.  The thickness in world units is
 * length * 2 r * 2^-24 whatever the length of d; overlapping spheres add.  f is the share of the sphere's OWN chord that lies inside the
 * window, so a sphere crossed whole counts as one diameter whatever the impact parameter (a disc splat, as a splatted thickness buffer
 * has it): through spheres of number density n the thickness per unit path is n pi r^2 * 2 r, three halves of the packing fraction
 * n 4 pi r^3 / 3.  Every field is a min, a max or an integer sum of per-sphere
 * values: the result does not depend on the order in which the spheres are met, is the same on every run, and sph_rays_span_host (brute
 * force) is its definition.  On rays that start outside every sphere, tEnter / idEnter are the cast's t / id.
 * SphRaySpansInfo: crossed (rays with count > 0), voidRays, total (the sum of count), maxCount: integer reductions.
 * Spans and hits are separate state: a span call does not end the held hits nor a cast the held spans; the spans stay valid until the
 * next sph_rays_span / _span_device, sph_reset or sph_destroy.  A span call changes no record.  Timed as SPH_K_OTHER.  Refusals, m = 0
 * and n = 0 as for the cast. */
typedef struct SphRaySpan { float tEnter, tExit; int32_t idEnter, idExit; uint32_t count, flags; uint64_t length; } SphRaySpan;   /* 32 bytes */
typedef struct SphRaySpansInfo { uint64_t rays, crossed, voidRays, total; uint32_t maxCount; float radius; int32_t flags; uint32_t pad; } SphRaySpansInfo;   /* 48 bytes */
/* m rays of 8 floats in HOST memory (may be null when m is 0): staged upload, then as _span_device.  Synchronises. */
int sph_rays_span(SphEngine* e, const float* rays8, size_t m, float radius, int flags, SphRaySpansInfo* out);
/* m rays of 8 floats in DEVICE memory (may be null when m is 0).  One synchronisation, for the four counts. */
int sph_rays_span_device(SphEngine* e, const float* devRays8, size_t m, float radius, int flags, SphRaySpansInfo* out);
/* What the engine holds. */
int sph_rays_span_info(const SphEngine* e, SphRaySpansInfo* out);
/* Borrowed device address: rows[rays]. */
int sph_rays_span_rows(SphEngine* e, const SphRaySpan** rows);
/* Copies the spans into the caller's memory, host or device (the kind of the copy follows from the address); synchronises. */
int sph_rays_span_download(SphEngine* e, SphRaySpan* rows);
/* Host-only, no device, THE DEFINITION: brute force over all participating records, no grid, the same ray_span.  rows may be null. */
int sph_rays_span_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                       SphRaySpan* rows, SphRaySpansInfo* out);
/* TEST HOOK.  Host-only, no device: the DEVICE's span walk (the same ray_span_walk function) over the grid as the counting sort leaves
 * it; variant 0 = the layer walk, 1 = the block walk.  Same bytes as sph_rays_span_host while the walk meets every sphere once. */
int sph_rays_span_walk_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                            int variant, SphRaySpan* rows, SphRaySpansInfo* out);

/* ---- free-surface particles (no reference counterpart) ---------------------------------------------------------
 * Which particles lie in the outer shell of the fluid, which way the surface faces there, and how sharply convex it is -- from the
 * positions alone, on the device.  Grid, radius rules (0 < R <= 3 cells), stencil, candidate order and r2 are those of the neighbour
 * lists above.  SphShellConfig: radius (<= 0: param_h), offset (the threshold, finite and >= 0, default 0.10), minCount (default 0 =
 * off), flags (SPH_SHELL_FLUID_ONLY: records with isGhost != 0 are never candidates and their own rows are all zero).
 * Pass 1, for a target at x: every accepted candidate j (r2 < R2; the target's own slot is left out by identity on particle rows), in
 * the order of the (2s + 1)^2 candidate rows, with d = x_j - x, t = R2 - r2, w = t * t:  count += 1, W += w, S = fmaf(w, d, S) per
 * axis.  Then s2 = dot3(S, S), lim = (offset * R) * W; the target is IN THE SHELL iff count == 0 or count < minCount or s2 > lim * lim;
 * normal = -S / sqrtf(s2) (zero where s2 == 0); offsetRatio = sqrtf(s2) / (R * W) (zero where W == 0); count == 0 also sets
 * SPH_SHELL_ISOLATED.  A target with a non-finite coordinate has an all-zero row.
 * Pass 2, particle rows only, for a shell particle i with normal n_i: every accepted shell candidate j != i in the same order with
 * dot3(d, n_i) < 0 (it lies behind i's tangent plane: the surface is convex there) adds the term (1 - dot3(n_i, n_j)) *
 * (1 - sqrtf(r2) / R), rounded once to fp32, to the crest sum -- the wave-crest sum of Ihmsen et al. 2012 over the shell.  The sum is
 * kept in fixed point (every term truncated to a multiple of 2^-32, int64 additions, one conversion to fp32 at the end), so crest does
 * not depend on the order of the candidates.  crest is 0 for rows that are not in the shell, for isolated rows and for query rows.  IEEE division and square root on both sides, every other operation rounded on its own
 * except the fmaf()s; no floating-point atomics: the same bytes on every run, and the bytes of sph_shell_host.
 * Outputs, engine-owned: rows SphShell[rows], numbered by particle id (or by query point), and ids int32[numShell], the rows in the
 * shell in ascending order (what a renderer gathers by).  SphShellInfo: numShell, numIsolated and maxCount (the largest count) are
 * integer reductions.  Query rows: pass 1 only, no own slot.
 * The buffers stay valid until the next sph_shell_build / _query, sph_reset or sph_destroy; neighbour lists, components, kNN rows and
 * ray hits have buffers of their own (no call of one kind invalidates another's); a dispatch does not touch them and a build never
 * changes the simulation.  Timed as SPH_K_OTHER.  SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as sampling); _info /
 * _device / _download before any build.  SPH_ERR_ARG: a null argument, a bad R, an offset that is not finite or < 0, unknown flag
 * bits, more than 2^31 - 1 query points.  n = 0 or m = 0: empty results, the call succeeds. */
enum { SPH_SHELL_FLUID_ONLY = 1 };                    /* SphShellConfig.flags */
enum { SPH_SHELL_MEMBER = 1, SPH_SHELL_ISOLATED = 2 };   /* SphShell.flags */
typedef struct SphShell { float normal[3]; float offsetRatio; float crest; uint32_t count; uint32_t flags; uint32_t pad; } SphShell;   /* 32 bytes */
typedef struct SphShellConfig { float radius; float offset; uint32_t minCount; int32_t flags; } SphShellConfig;   /* 16 bytes */
typedef struct SphShellInfo { uint64_t rows, numShell, numIsolated; uint32_t maxCount; float radius; int32_t stencil, kind /*0 none, 1 particles, 2 query*/, flags; uint32_t pad; } SphShellInfo;   /* 48 bytes */
/* radius 0 (param_h), offset 0.10, minCount 0, flags 0. */
void sph_shell_default(SphShellConfig* cfg);
/* Rows of every particle, both passes.  Synchronises. */
int sph_shell_build(SphEngine* e, const SphShellConfig* cfg, SphShellInfo* out);
/* Rows of m query points of 4 floats (x, y, z, unused) in DEVICE memory (may be null when m is 0), pass 1 only.  Synchronises. */
int sph_shell_query(SphEngine* e, const float* devPoints4, size_t m, const SphShellConfig* cfg, SphShellInfo* out);
/* What the engine holds. */
int sph_shell_info(const SphEngine* e, SphShellInfo* out);
/* Borrowed device addresses: rows[rows], ids[numShell]. */
int sph_shell_device(SphEngine* e, const SphShell** rows, const int32_t** ids);
/* Copies into the caller's memory, host or device (the kind of each copy follows from the address); synchronises; either pointer may
 * be null. */
int sph_shell_download(SphEngine* e, SphShell* rows, int32_t* ids);
/* Host-only, no device: the counting sort of sph_neighbors_host and the same per-candidate, finish and crest functions in the same
 * order; the same bytes.  points4 NULL: particle rows of particles[0 .. n) (m ignored); else query rows of m points.  rows and ids
 * (room for one entry per row) may be null; so may sums4, which receives the sums of pass 1 the rows were finished from, 4 floats per
 * row (Sx, Sy, Sz, W) -- what the tests hold against a float64 restatement. */
int sph_shell_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m, const SphShellConfig* cfg,
                   SphShell* rows, int32_t* ids, float* sums4, SphShellInfo* out);

/* ---- anisotropic kernels (no reference counterpart) -------------------------------------------------------------
 * Per particle a smoothed centre and an ellipsoid from the weighted covariance of its neighbourhood (Yu & Turk 2013), and the lattice
 * of the anisotropic fraction summed from those ellipsoids, whose iso-surface is flatter on flat water and thinner on sheets than the
 * surface of SPH_FIELD_FRACTION.  Grid, radius rules (0 < R <= 3 cells), stencil, candidate order and r2 are those of the neighbour
 * lists above.  SphAnisoConfig: radius R (<= 0: 2 * param_h), support a (<= 0: param_h; finite), smoothing lambda (0 .. 1), maxRatio kr
 * (finite, >= 1), maxStretch (finite, > 0), sparseScale kn (finite, > 0), minCount, flags (SPH_ANISO_FLUID_ONLY: records with
 * isGhost != 0 are never candidates and their own rows are all zero).
 * Sums, for a particle at x over every accepted candidate j (r2 < R2; the particle's own slot is one of them: d = 0) in the order of
 * the (2s + 1)^2 candidate rows, with d = x_j - x, t = R2 - r2, w = (t * t) * t:  count += 1, W += w, S_a = fmaf(w, d_a, S_a),
 * M_ab = fmaf(w * d_a, d_b, M_ab) for ab in xx, yy, zz, xy, xz, yz.
 * Finish: m_a = S_a / W; C_ab = (M_ab / W - m_a * m_b) * (11.0f / R2) (the identity for a full, uniformly filled neighbourhood); C is
 * eigen-decomposed by five sweeps of cyclic Jacobi over the pairs (0,1), (0,2), (1,2) (a step is skipped when a_pq == 0; th = (a_qq -
 * a_pp) / (2 a_pq), t = 1 / (|th| + sqrtf(th * th + 1)) negated when th < 0, c = 1 / sqrtf(t * t + 1), s = t * c, a_pp -= t a_pq,
 * a_qq += t a_pq, a_pq = 0, the remaining pair and the columns of V rotated as (x, y) -> (fmaf(-s, y, c * x), fmaf(s, x, c * y))); the
 * eigenvalues are sorted in descending order by the exchanges (0,1), (1,2), (0,1) with a strict compare, columns with them;
 * s_k = sqrtf(max(l_k, 0)).  The row is SPARSE if count < minCount or !(s_0 > 0): then s = (kn, kn, kn) and the axes are the coordinate
 * axes.  Otherwise s_0 = min(s_0, maxStretch), s_k = min(max(s_k, s_0 / kr), maxStretch), and the row is CLAMPED if any s_k changed.
 * Row (SphAniso, 64 bytes, numbered by particle id): center = fmaf(lambda, m, x); axisK = (a * s_k) * v_k, the ellipsoid's semi-axis
 * vectors in world units, longest first (their handedness is not fixed); reach = a * s_0 + |center - x|: how far from the particle's
 * own position its ellipsoid can be met; amplitude = invRho * ((i_0 * i_1) * i_2), i_k = 1 / (a * s_k), invRho the word the fraction
 * sampler reads (density > 0 ? 1.0f / density : 0.0f).  A particle with a non-finite position has an all-zero row (no SPH_ANISO_VALID)
 * and is never a candidate; under SPH_ANISO_FLUID_ONLY so has a ghost.
 * Field: a lattice node at x = origin + (float)i * spacing (x fastest, the coordinates of sph_sample_lattice) walks the candidate rows
 * at reachStencil = the stencil of the largest reach around its cell; per candidate r = x - center_j, skipped unless dot3(r, r) <
 * (a * s_0)^2; q2 = r' Q r with Q = sum_k (i_k * i_k) v_k v_k'; u = max(1 - q2, 0); acc = fmaf(amplitude_j, (u * u) * u, acc); the
 * node's value is (param_mass * 1.5666815f) * acc (315 / (64 pi)); a node with a non-finite coordinate gets 0.  With every s_k = 1 and
 * a = h this is SPH_FIELD_FRACTION up to rounding.  If the largest reach exceeds three cells, sph_aniso_lattice and sph_aniso_surface
 * refuse with SPH_ERR_ARG ("maxReach ..."): the rows of that build are still held (sph_aniso_info says how large it was); lower
 * support, maxStretch or smoothing.
 * IEEE division and square root on both sides, every other operation rounded on its own except the fmaf()s (csrc/sph_aniso.h lists
 * them); no floating-point atomics: the same bytes on every run, and the bytes of sph_aniso_host / sph_aniso_lattice_host.
 * The rows are the engine's own and stay valid until the next sph_aniso_build / _lattice / _surface, sph_reset or sph_destroy; no
 * other family invalidates them, a dispatch does not touch them and a build never changes the simulation.  Timed as SPH_K_OTHER.
 * SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as sampling); _info / _device / _download before any build.  SPH_ERR_ARG: a
 * null argument, a config value outside its range, unknown flag bits, a negative lattice dimension, a spacing that is not finite or
 * <= 0, more than 2^31 - 1 nodes.  n = 0 and a lattice with a dimension of 0: empty results, the call succeeds. */
enum { SPH_ANISO_FLUID_ONLY = 1 };                    /* SphAnisoConfig.flags */
enum { SPH_ANISO_VALID = 1, SPH_ANISO_SPARSE = 2, SPH_ANISO_CLAMPED = 4 };   /* SphAniso.flags */
typedef struct SphAniso { float center[3]; uint32_t count; float axis0[3]; uint32_t flags; float axis1[3]; float reach; float axis2[3]; float amplitude; } SphAniso;   /* 64 bytes */
typedef struct SphAnisoConfig { float radius, support, smoothing, maxRatio, maxStretch, sparseScale; uint32_t minCount; int32_t flags; } SphAnisoConfig;   /* 32 bytes */
typedef struct SphAnisoInfo { uint64_t rows, numSparse, numClamped; uint32_t maxCount; float radius, support; int32_t stencil; float maxReach; int32_t reachStencil /*0: no reach, or above three cells*/, kind /*0 none, 1 particles*/, flags; } SphAnisoInfo;   /* 56 bytes */
/* radius 0 (2 * param_h), support 0 (param_h), smoothing 0.9, maxRatio 4, maxStretch 1.5, sparseScale 0.5, minCount 25, flags 0. */
void sph_aniso_default(SphAnisoConfig* cfg);
/* Rows of every particle.  Synchronises. */
int sph_aniso_build(SphEngine* e, const SphAnisoConfig* cfg, SphAnisoInfo* out);
/* What the engine holds. */
int sph_aniso_info(const SphEngine* e, SphAnisoInfo* out);
/* Borrowed device address: rows[rows] (what a splat renderer binds). */
int sph_aniso_device(SphEngine* e, const SphAniso** rows);
/* Copies into the caller's memory, host or device (the kind of the copy follows from the address); synchronises. */
int sph_aniso_download(SphEngine* e, SphAniso* rows);
/* Builds the rows (as sph_aniso_build, one read-back of the info), then writes dims[0] * dims[1] * dims[2] floats to devOut in DEVICE
 * memory, asynchronously on the engine's stream. */
int sph_aniso_lattice(SphEngine* e, const SphAnisoConfig* cfg, const float origin[3], const float spacing[3], const int dims[3], float* devOut, SphAnisoInfo* out);
/* The lattice into engine scratch, then the mesher of sph_extract_surface_volume: {value >= iso} as a closed triangle mesh (dims >= 2
 * per axis).  `out` borrows from the engine under the rules of sph_extract_surface; sph_surface_download copies it. */
int sph_aniso_surface(SphEngine* e, const SphAnisoConfig* cfg, const float origin[3], const float spacing[3], const int dims[3], float iso, SphSurface* out,
                      SphAnisoInfo* info);
/* Host-only, no device: the counting sort of sph_neighbors_host and the same sum, finish and node functions in the same order; the
 * same bytes.  rows (n records) may be null. */
int sph_aniso_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAnisoConfig* cfg, SphAniso* rows, SphAnisoInfo* out);
/* The twin of sph_aniso_lattice: values (dims[0] * dims[1] * dims[2] floats, x fastest) in host memory. */
int sph_aniso_lattice_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAnisoConfig* cfg, const float origin[3],
                           const float spacing[3], const int dims[3], float* values, SphAnisoInfo* out);

/* ---- fused neighbourhood reductions of caller tensors (no reference counterpart) -------------------------------
 * Sum, mean, maximum or minimum of a caller's per-particle tensor values[n][C] (float32, row-major by particle id, device memory, never
 * written) over the neighbours of every particle (rows numbered by particle id) or of m query points (x, y, z, .).  A query: it keeps
 * no result and no engine state.  Grid, radius rules (0 < R <= 3 cells), stencil and candidate order (ascending sorted slot = ascending
 * (cell index, particle id)) are those of the neighbour lists above; candidate j is accepted when r2 < R2 with d = x_j - x_i,
 * r2 = dot3(d, d) (the bits of the lists' r2).  1 <= channels <= SPH_AGGREGATE_MAX_CHANNELS.
 * Flags.  SELF (particle targets): the own slot is kept by slot identity and enters with d = 0, r2 = 0 exactly; without it the own slot
 * is skipped.  FLUID_ONLY: records with isGhost != 0 are never candidates and a ghost target has an empty row.  DELTA (particle targets):
 * the reduced value is values[j][c] - values[i][c], one rounded subtraction.  MOMENTS (SUM only): see below.  A query point with a
 * non-finite coordinate has an empty row; a particle with a non-finite position accepts nobody and is accepted by nobody, so its row
 * is empty apart from its own slot under SELF.
 * Weights.  ONE: w = 1.  POLY6: t = R2 - r2, w = (t * t) * t, unnormalised.
 * Operations, per channel one fp32 accumulator over the accepted candidates in the order above, every product and sum rounded on its
 * own (no fused multiply-add anywhere): SUM acc = acc + w * v.  MEAN the same and W = W + w; the result is acc / W (IEEE division), +0
 * where W == 0.  MAX / MIN (weight ONE): compared through the ordered-bits key of the fp32 value (the key of the rays' t), so -0 < +0
 * and the result does not depend on the order; a NaN never wins; an empty row is -inf for MAX and +inf for MIN.  MOMENTS: the output row
 * is [4][C]; plane 0 is the SUM, planes 1 .. 3 are acc_a = acc_a + (w * d_a) * v for a = x, y, z (with DELTA the raw sums an SPH
 * gradient, divergence or curl of the caller's field is assembled from).  NaN and inf values propagate through SUM and MEAN in the rows
 * that accept them, and in no other row.
 * Outputs, device memory: out float32[rows][planes][C] (planes 1, or 4 with MOMENTS); count (may be null) uint32[rows], the candidates
 * reduced: for particle targets the degree sph_neighbors_build(SPH_NEIGHBORS_COUNT_ONLY) gives at the same radius and SELF setting,
 * under FLUID_ONLY the non-ghost ones of them.  The same bytes on every run, and the bytes of sph_aggregate_host.
 * The device calls work on the engine's stream and do NOT synchronise: out and count are complete once the stream has drained
 * (sph_sync), and values must stay unchanged until then; a caller that fills values on another stream synchronises that stream first.
 * A later dispatch is unaffected, a call never changes the simulation.  Timed as SPH_K_OTHER.
 * SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1 (as sampling), before any allocation.  SPH_ERR_ARG: a null argument, a radius
 * that is not finite, <= 0 or above three cells, an unknown op, weight or flag bit, non-zero padding, channels outside 1 .. 128, MOMENTS
 * without SUM, MAX / MIN with POLY6, SELF or DELTA on query targets, more than 2^31 - 1 query points, out or count overlapping values
 * as address ranges, rows * planes * channels beyond size_t.  m = 0 or n = 0: success, nothing is written. */
enum { SPH_AGGREGATE_SUM = 0, SPH_AGGREGATE_MEAN = 1, SPH_AGGREGATE_MAX = 2, SPH_AGGREGATE_MIN = 3 };                  /* SphAggregateConfig.op */
enum { SPH_AGGREGATE_WEIGHT_ONE = 0, SPH_AGGREGATE_WEIGHT_POLY6 = 1 };                                                 /* SphAggregateConfig.weight */
enum { SPH_AGGREGATE_SELF = 1, SPH_AGGREGATE_FLUID_ONLY = 2, SPH_AGGREGATE_DELTA = 4, SPH_AGGREGATE_MOMENTS = 8 };     /* SphAggregateConfig.flags */
enum { SPH_AGGREGATE_MAX_CHANNELS = 128 };
typedef struct SphAggregateConfig { float radius; int32_t op, weight, flags, channels; int32_t pad[3]; } SphAggregateConfig;   /* 32 bytes */
typedef struct SphAggregateInfo { uint64_t rows; int32_t channels, planes, stencil, flags; float radius; int32_t pad; } SphAggregateInfo;   /* 32 bytes */
/* radius 0 (to be set: there is no default radius), op SUM, weight ONE, flags 0, channels 1, padding 0. */
void sph_aggregate_default(SphAggregateConfig* cfg);
/* Rows of every particle: devValues float32[n][channels], devOut float32[n][planes][channels], devCount uint32[n] or null. */
int sph_aggregate_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, SphAggregateInfo* info);
/* Rows of m query points (x, y, z, .) in device memory: devOut float32[m][planes][channels], devCount uint32[m] or null. */
int sph_aggregate_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                        uint32_t* devCount, SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets; count may be null): values, and the points, are uploaded
 * into engine scratch, out and count are copied back; synchronises. */
int sph_aggregate_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* values, float* out, uint32_t* count,
                         SphAggregateInfo* info);
/* Host-only, no device: the counting sort of sph_neighbors_host and the same per-candidate functions in the same order; the same bytes.
 * points4 null: particle targets.  count may be null. */
int sph_aggregate_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                       const float* values, float* out, uint32_t* count);

/* ---- the adjoint of the neighbourhood sums, and extrema that say who won (no reference counterpart) -------------
 * Every SUM above is a linear map A of values whose weights depend on the engine's positions alone; these calls apply its exact
 * transpose.  Config: SphAggregateConfig under the rules above, op SUM.  Input g float32[rows][planes][C], what the forward's out would
 * be (rows = n, or m for query targets; planes 4 with MOMENTS); output out float32[n][C] by particle id.  Every row of out is written,
 * +0 where nothing contributes.  Queries like the forward: no result is kept, no engine state, nothing in a checkpoint.
 * Definition.  Particle k sums over the rows i that accept k in the forward, with the forward's own bits of d = x_k - x_i (row i's
 * offset to candidate k, the same operand order), r2 and w.  Order of the rows: particle targets ascending sorted slot (the forward's
 * candidate order); query targets ascending (clamped cell index of the point, point index).  One fp32 accumulator per channel; per row
 * and channel, in this order, every product and sum rounded on its own:
 *   without DELTA   acc = acc + w * g[i][0][c];                          with MOMENTS then, a = x, y, z: acc = acc + (w * d_a) * g[i][1+a][c]
 *   with DELTA      acc = acc + w * (g[i][0][c] - g[k][0][c]);           with MOMENTS then: acc = acc + (w * d_a) * (g[i][1+a][c] + g[k][1+a][c])
 * (the moment planes under DELTA: the derivative of sum_j (w d_a)(x_j - x_i) with respect to x_k; the two occurrences of x_k combine
 * because d is antisymmetric and w * d negates exactly).  The forward's rules hold transposed: under SELF the own slot enters by slot
 * identity with d = 0; under FLUID_ONLY a ghost particle's row of out is zero and a ghost target's row of g contributes nothing; a
 * particle with a non-finite position has a zero row apart from its own slot under SELF; a query point with a non-finite coordinate
 * contributes nothing.
 * Why the rows found are the transpose: the stencil is a box of cells, symmetric per axis, and both sides use clamped cells, so "the
 * row's cell lies in my stencil" is exactly "my cell lies in the row's stencil"; acceptance itself (r2 < R2, slot identity, the ghost
 * rules) reads the same bits from either side.
 * Identity: for particle targets without MOMENTS the call gives, byte for byte, sph_aggregate_particles(cfg, g), with and without
 * DELTA, SELF and FLUID_ONLY (the relation and the weights are symmetric); the library runs that kernel.  SPH_OPT_AGGREGATE_VARIANT
 * steers it there and nothing else here; the bytes do not move.
 * Query targets bin the m points into the engine's grid by their clamped cell, in (cell, point index) order without the non-finite
 * ones (a counting sort whose arrival order a ranking pass removes), stage g into that order, and one particle per lane walks the
 * forward's stencil around its own clamped cell over the points' cell table.  No float atomics; stores are lane-owned.  The same
 * bytes on every run, and the bytes of sph_aggregate_adjoint_host, which runs the same per-term functions in the same order.
 * Streams, timing class and SPH_ERR_STATE as the forward.  SPH_ERR_ARG: the forward's cases, and op != SUM, a null g or out, out
 * overlapping g or the points as address ranges.  m = 0: out is zeroed.  n = 0: success, nothing is written.
 * SphAggregateInfo: rows = n (the rows of out), planes those of g. */
int sph_aggregate_adjoint_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devG, float* devOut, SphAggregateInfo* info);
/* devPoints4: m query points (x, y, z, .) in device memory, never written; devG float32[m][planes][channels]. */
int sph_aggregate_adjoint_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devG, float* devOut,
                                SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets): g, and the points, are uploaded into engine scratch,
 * out is copied back; synchronises. */
int sph_aggregate_adjoint_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* g, float* out,
                                 SphAggregateInfo* info);
/* Host-only, no device: the same bytes.  points4 null: particle targets. */
int sph_aggregate_adjoint_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                               const float* g, float* out);
/* MAX / MIN (any other op: SPH_ERR_ARG) with one more output, arg int32[rows][C]: out and count are byte for byte those of
 * sph_aggregate_particles / _query; arg[i][c] is the smallest particle id among the accepted candidates whose reduced value is not NaN
 * and whose ordered key equals the winning key, -1 for an empty row or a row of NaNs.  Coincident particles and lattices therefore have
 * one answer, whatever the order of the walk.  Further SPH_ERR_ARG: a null arg, outputs that overlap the values or each other. */
int sph_aggregate_arg_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, int32_t* devArg,
                                SphAggregateInfo* info);
int sph_aggregate_arg_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                            uint32_t* devCount, int32_t* devArg, SphAggregateInfo* info);
int sph_aggregate_arg_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                           const float* values, float* out, uint32_t* count, int32_t* arg);
/* The routing of a gradient through MAX / MIN (config as for arg): out[k][c] is the sum, in the adjoint's row order, of g[i][c] over the
 * rows i that accept k with arg[i][c] == k; the step is acc = acc + g.  arg int32[rows][C] and g float32[rows][C] are never written; out
 * float32[n][C], every row written.  A winner is always an accepted candidate, so the adjoint's walk finds every such row: a gather,
 * no scatter.  Refusals as the adjoint's (op MAX or MIN), and a null arg or out overlapping arg. */
int sph_aggregate_route_particles(SphEngine* e, const SphAggregateConfig* cfg, const int32_t* devArg, const float* devG, float* devOut, SphAggregateInfo* info);
int sph_aggregate_route_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const int32_t* devArg, const float* devG,
                              float* devOut, SphAggregateInfo* info);
int sph_aggregate_route_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                             const int32_t* arg, const float* g, float* out);

/* ---- filter-grid basis sums: continuous convolutions without an edge list (no reference counterpart) -----------
 * A continuous convolution (Ummenhofer et al. 2020) interpolates a K x K x K grid of Cin x Cout filter matrices trilinearly at the
 * neighbour's offset, so it is linear in B = K^3 fixed geometric functions.  These calls give the basis sums
 *   A[i][b][c] = sum_j w(r_ij) * phi_b(x_j - x_i) * values[j][c]
 * of a caller's values[n][C] (float32, row-major by particle id, device memory, never written) over the neighbours of every particle or
 * of m query points; the learned part is one dense product A.reshape(rows, B * C) @ filters.reshape(B * C, Cout) that the caller runs.
 * A query: it keeps no result, puts nothing in a checkpoint and touches no engine state.
 * Grid, radius rules (0 < R <= 3 cells), stencil, candidate order (ascending sorted slot), acceptance (d = x_j - x_i, r2 < R2), SELF by
 * slot identity with d = 0, FLUID_ONLY, and the empty rows of non-finite targets and points are those of the fused neighbourhood
 * reductions above.  Not supported, SPH_ERR_ARG: DELTA, MOMENTS (any flag bit but SELF and FLUID_ONLY); the operation is SUM.  Weights:
 * SPH_AGGREGATE_WEIGHT_ONE, or _POLY6 (t = R2 - r2, w = (t * t) * t).
 * Config.  kind SPH_BASIS_GRID (the only one), size = K in {2, 3, 4}, 1 <= channels <= SPH_AGGREGATE_MAX_CHANNELS, zero padding.
 * Coordinates, per axis a, every operation fp32 and rounded on its own (no fused multiply-add):
 *   u_a = d_a / R (IEEE division by the config's radius);  g_a = (u_a + 1.0f) * half, half = 0.5f * (float)(K - 1);
 *   i_a = (int)g_a clamped to [0, K - 2];  f_a = g_a - (float)i_a;  lo_a = 1.0f - f_a;  hi_a = f_a
 * the linear map of [-R, R] onto the grid's [0, K - 1] with aligned corners and no ball-to-cube map (|d_a| < R for an accepted
 * candidate, so the clamp is a guard).  Per candidate the 8 corners (cz, cy, cx) in {lo, hi}^3 have the plane index
 * b = ((i_z + cz) K + (i_y + cy)) K + (i_x + cx), x fastest, the coefficient coef = w * ((wx * wy) * wz) and the step
 * acc[b][c] = acc[b][c] + coef * v[c], zero coefficients included.  The 8 planes are distinct, so the order of the corners does not
 * enter the bytes.  NaN and inf values propagate in the rows that accept them.
 * Outputs, device memory: out float32[rows][B][C], c fastest, every row written (+0 where empty); count (may be null) uint32[rows],
 * the numbers sph_aggregate_* gives.  The same bytes on every run, and the bytes of sph_aggregate_basis_host.
 * Adjoint.  Input h float32[rows][B][C], output out float32[n][C] by particle id, every row written.  Particle k sums over the rows i
 * that accept it in the order of sph_aggregate_adjoint_* (particle targets: ascending sorted slot; query targets: ascending (clamped
 * cell of the point, point index)), with the forward's own bits of d = x_k - x_i, r2, w and the corner coefficients; per row the 8
 * corners in ascending b: acc = acc + coef_b * h[i][b][c].  Query targets are binned as there.  No float atomics; the same bytes on
 * every run, and the bytes of sph_aggregate_basis_adjoint_host.
 * Streams: the device calls work on the engine's stream and do NOT synchronise; timed as SPH_K_OTHER.  SphAggregateInfo: rows (those
 * of out), channels, planes = B, stencil, flags, radius.
 * SPH_ERR_STATE: z-slab engines and SPH_OPT_GRID_BUILD 1, before any allocation.  SPH_ERR_ARG: a null argument, a bad radius, an
 * unknown weight, kind or flag bit (DELTA and MOMENTS among them), a size outside 2 .. 4, channels outside 1 .. 128, non-zero padding,
 * SELF on query targets, more than 2^31 - 1 query points, overlapping address ranges (out or count with values; the adjoint's out with
 * h or the points), rows * B * channels beyond size_t.  Forward, m = 0 or n = 0: success, nothing is written.  Adjoint, m = 0: out is
 * zeroed; n = 0: success, nothing is written. */
enum { SPH_BASIS_GRID = 0 };                                                                                            /* SphBasisConfig.kind */
typedef struct SphBasisConfig { float radius; int32_t weight, flags, channels, kind, size; int32_t pad[2]; } SphBasisConfig;     /* 32 bytes */
/* radius 0 (to be set), weight POLY6, flags 0, channels 1, kind GRID, size 4, padding 0. */
void sph_aggregate_basis_default(SphBasisConfig* cfg);
/* Rows of every particle: devValues float32[n][channels], devOut float32[n][B][channels], devCount uint32[n] or null. */
int sph_aggregate_basis_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, SphAggregateInfo* info);
/* Rows of m query points (x, y, z, .) in device memory: devOut float32[m][B][channels], devCount uint32[m] or null. */
int sph_aggregate_basis_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                              uint32_t* devCount, SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets; count may be null); synchronises. */
int sph_aggregate_basis_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* values, float* out, uint32_t* count,
                               SphAggregateInfo* info);
/* Host-only, no device: the same per-candidate functions in the same order; the same bytes.  points4 null: particle targets. */
int sph_aggregate_basis_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                             const float* values, float* out, uint32_t* count);
/* The adjoint: devH float32[rows][B][channels], devOut float32[n][channels]. */
int sph_aggregate_basis_adjoint_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devH, float* devOut, SphAggregateInfo* info);
int sph_aggregate_basis_adjoint_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devH, float* devOut,
                                      SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets); synchronises. */
int sph_aggregate_basis_adjoint_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* h, float* out,
                                       SphAggregateInfo* info);
/* Host-only, no device: the same bytes.  points4 null: particle targets. */
int sph_aggregate_basis_adjoint_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                                     const float* h, float* out);

/* ---- position gradients of the neighbourhood sums (no reference counterpart) -----------------------------------
 * The SUM of sph_aggregate_* as a function of the POSITIONS: with values float32[n][C] (the forward's input) and g float32[rows][planes][C]
 * (the upstream gradient: what the forward's out would be, as the adjoint takes it), the scalar is L = sum g . out, and these calls give
 * dL/dx of the particles and, for query targets, of the query points.  Config: SphAggregateConfig under the forward's rules, op SUM
 * (MEAN is composed above this layer), weight ONE or POLY6, any of SELF, FLUID_ONLY, DELTA, MOMENTS.  A query: no result is kept, no
 * engine state is written, nothing enters a checkpoint.
 * The pair term.  For a target i (a particle or a query point) and a candidate j that the forward accepts, with the forward's own bits
 * of d = x_j - x_i, r2 and w, every product and sum fp32 and rounded on its own (no fused multiply-add):
 *   val_c = v[j][c], with DELTA v[j][c] - v[i][c]                          (the forward's reduced value)
 *   s_p   = sum_c g[i][p][c] * val_c, p = 0 .. planes - 1                  (the channel dot, order below)
 *   w1    = 0 for ONE;  POLY6: t = R2 - r2, w1 = -6.0f * (t * t)
 *   q     = s_0;  with MOMENTS q = ((s_0 + d_x * s_1) + d_y * s_2) + d_z * s_3
 *   f     = w1 * q;  e_a = f * d_a;  with MOMENTS e_a = (f * d_a) + w * s_{1+a},  a = x, y, z
 * e(i -> j) is dL/dd of that pair: it goes to x_j with + and to x_i with -.
 * Order of the channel dot, a function of C alone: G = the smallest of 4, 8, 16, 32, 64 that holds C (64 for C > 64).  Lane l of G
 * sums the channels c = l, l + G, .. ascending, part = part + g * val from +0 (+0 where it has no channel); then for off = 1, 2, 4, ..
 * G / 2 every lane takes part[l] = part[l] + part[l xor off] (all lanes at once).  Every lane ends with the same bits; they are s_p.
 * Particle targets, one output grad float32[n][3] by particle id: grad[k] = sum over k's accepted candidates j != k in ascending sorted
 * slot of (e(j -> k) - e(k -> j)), acc_a = acc_a + (eIn_a - eOut_a) from +0.  e(k -> j) uses g[k] and val = v[j] (- v[k]) with d; e(j -> k)
 * uses g[j] and val = v[k] (- v[j]) with -d (exact), the same r2 and w.  The relation is symmetric, so this one walk meets every pair
 * that involves k.  Under SELF the own slot contributes nothing (its two terms are equal) and is skipped: SELF does not move a byte.
 * Query targets, two outputs: gradPoints float32[m][3], row i = the sum over the row's accepted candidates in the forward's order,
 * acc_a = acc_a - e_a(i -> j) from +0; gradParticles float32[n][3], row k = the sum over the rows i that accept k in the adjoint's row
 * order (ascending (clamped cell of the point, point index)), acc_a = acc_a + e_a(i -> k), the points binned as there.  Either may be
 * null: its walk is not launched.
 * The forward's rules carry over: under FLUID_ONLY a ghost is neither a target nor a candidate, its rows are +0; a particle or a query
 * point with a non-finite coordinate has +0 rows and contributes to nobody.  Every row of every output is written.  Weight ONE
 * without MOMENTS does not depend on the positions: the outputs are zeroed without a walk, after the argument and state checks.
 * The cutoff itself is not differentiated: the jump of ONE and of the moment planes at r = R is ignored, as every fixed-radius
 * operator does; POLY6 and its derivative vanish there, so for POLY6 without MOMENTS the gradient is the true one.
 * No float atomics; stores are lane-owned.  The same bytes on every run, and the bytes of sph_aggregate_posgrad_host, which runs the
 * same per-term functions in the same order.  SPH_OPT_AGGREGATE_VARIANT does not reach these calls.
 * Streams, the timing class (SPH_K_OTHER) and SPH_ERR_STATE (z-slab engines, SPH_OPT_GRID_BUILD 1; before any allocation) as the
 * adjoint.  SPH_ERR_ARG: the adjoint's cases, a null values, an output that overlaps values, g, the points or the other output as
 * address ranges, both query outputs null.  m = 0: gradParticles is zeroed.  n = 0: success, nothing is written.
 * SphAggregateInfo: rows = those of g (n, or m), planes those of g. */
/* Particle targets: devValues float32[n][channels], devG float32[n][planes][channels], devOut float32[n][3]. */
int sph_aggregate_posgrad_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, const float* devG, float* devOut, SphAggregateInfo* info);
/* devPoints4: m query points (x, y, z, .) in device memory, never written; devG float32[m][planes][channels]; devOutPoints float32[m][3]
 * or null; devOutParticles float32[n][3] or null. */
int sph_aggregate_posgrad_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                float* devOutPoints, float* devOutParticles, SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets, outPoints is not read); synchronises. */
int sph_aggregate_posgrad_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* values, const float* g, float* outPoints,
                                 float* outParticles, SphAggregateInfo* info);
/* Host-only, no device: the same bytes.  points4 null: particle targets (outPoints is not read). */
int sph_aggregate_posgrad_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                               const float* values, const float* g, float* outPoints, float* outParticles);

/* ---- position gradients of the basis sums (no reference counterpart) --------------------------------------------
 * The basis sums of sph_aggregate_basis_* as a function of the POSITIONS: with values float32[n][C] (the forward's input) and
 * g float32[rows][B][C] (the upstream gradient: what the forward's out would be, as the basis adjoint takes its h), the scalar is
 * L = sum g . out, and these calls give dL/dx of the particles and, for query targets, of the query points.  Config: SphBasisConfig
 * under the forward's rules.  A query: no result is kept, no engine state is written, nothing enters a checkpoint.
 * The pair term.  For a target i (a particle or a query point) and a candidate j != i that the forward accepts, with the forward's own
 * bits of d = x_j - x_i, r2 and w, every product and sum fp32 and rounded on its own (no fused multiply-add):
 *   per axis a: the forward's u = d_a / R, g_a = (u + 1) * half, cell i_a, f = g_a - i_a, hat weights lo_a = 1 - f, hi_a = f; their slopes
 *               are -s and +s, s = half / R (one division): the derivative of the linear piece the forward selects
 *   corner n = 0 .. 7 (cx = n & 1, cy = (n >> 1) & 1, cz = n >> 2; plane b_n as the forward), w_a / s_a the hat weight / slope of the
 *               corner's side of axis a:
 *               hat_n = (w_x * w_y) * w_z   (without w)
 *               dx_n  = (s_x * w_y) * w_z,  dy_n = (w_x * s_y) * w_z,  dz_n = (w_x * w_y) * s_z
 *   a lane's partial sums, G = the smallest of 4, 8, 16, 32, 64 that holds C (64 for C > 64): lane l of G starts pq, px, py, pz at +0
 *               and takes its channels c = l, l + G, .. ascending, inside a channel the corners n = 0 .. 7 ascending:
 *               u = g[i][b_n][c] * v[j][c];  pq = pq + hat_n * u;  pa = pa + da_n * u  (a = x, y, z)
 *               (one running sum over all the lane's channels and corners; a lane without a channel keeps +0)
 *   then for off = 1, 2, 4, .. G / 2 every lane takes part[l] = part[l] + part[l xor off] (all lanes at once), each of the four sums on
 *               its own.  Every lane ends with the same bits: q, p_x, p_y, p_z.
 *   w1 = 0 for ONE;  POLY6: t = R2 - r2, w1 = -6.0f * (t * t);  f = w1 * q;  e_a = (f * d_a) + w * p_a
 * e(i -> j) is dL/dd of that pair: it goes to x_j with + and to x_i with -.  The kink of a hat at an integer g_a and the cutoff at r = R
 * are not differentiated (POLY6 vanishes at the cutoff; ONE jumps there, as for every fixed-radius operator).  Weight ONE still
 * depends on the positions through the hats: there is no zeroed shortcut.
 * Particle targets, one output grad float32[n][3] by particle id: grad[k] = sum over k's accepted candidates j != k in ascending sorted
 * slot of (e(j -> k) - e(k -> j)), acc_a = acc_a + (eIn_a - eOut_a) from +0.  e(k -> j) uses g[k], v[j] and d; e(j -> k) uses g[j], v[k]
 * and -d (exact), the same r2 and w, its cells and hat weights from the per-axis rule applied to -d (not mirrored from d).  Under SELF
 * the own slot's d = x_k - x_k moves with no position and is skipped: SELF does not move a byte.
 * Query targets, two outputs: gradPoints float32[m][3], row i = the sum over the row's accepted candidates in the forward's order,
 * acc_a = acc_a - e_a(i -> j) from +0; gradParticles float32[n][3], row k = the sum over the rows i that accept k in the adjoint's row
 * order (ascending (clamped cell of the point, point index)), acc_a = acc_a + e_a(i -> k), the points binned as there.  Either may be
 * null: its walk is not launched.
 * The forward's rules carry over: under FLUID_ONLY a ghost is neither a target nor a candidate, its rows are +0; a particle or a query
 * point with a non-finite coordinate has +0 rows and contributes to nobody.  Every row of every output is written.
 * No float atomics; stores are lane-owned.  The same bytes on every run, and the bytes of sph_aggregate_basis_posgrad_host, which runs
 * the same per-term functions in the same order.
 * Streams, the timing class (SPH_K_OTHER) and SPH_ERR_STATE (z-slab engines, SPH_OPT_GRID_BUILD 1; before any allocation) as the basis
 * sums.  SPH_ERR_ARG: the basis sums' cases (a bad weight, flags, channels, kind, size or radius, SELF on query targets, m >= 2^31, a
 * null argument), an output that overlaps values, g, the points or the other output as address ranges, both query outputs null.
 * m = 0: gradParticles is zeroed.  n = 0: success, nothing is written.  SphAggregateInfo: rows = those of g (n, or m), planes = B. */
/* Particle targets: devValues float32[n][channels], devG float32[n][B][channels], devOut float32[n][3]. */
int sph_aggregate_basis_posgrad_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devValues, const float* devG, float* devOut, SphAggregateInfo* info);
/* devPoints4: m query points (x, y, z, .) in device memory, never written; devG float32[m][B][channels]; devOutPoints float32[m][3] or
 * null; devOutParticles float32[n][3] or null. */
int sph_aggregate_basis_posgrad_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                      float* devOutPoints, float* devOutParticles, SphAggregateInfo* info);
/* The same two calls for arrays in HOST memory (points4 null: particle targets, outPoints is not read); synchronises. */
int sph_aggregate_basis_posgrad_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* values, const float* g,
                                       float* outPoints, float* outParticles, SphAggregateInfo* info);
/* Host-only, no device: the same bytes.  points4 null: particle targets (outPoints is not read). */
int sph_aggregate_basis_posgrad_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                                     const float* values, const float* g, float* outPoints, float* outParticles);

/* ---- multi-GPU: z-slab decomposition (no reference counterpart) ------------
 * One engine per rank owns the global cell layers [z0, z1) of ComputeGridExtents' grid plus one
 * read-only ghost layer per side.  Per substep the host calls pack -> (exchange) -> unpack ->
 * sph_dispatch.  Records crossing ranks are 64 bytes: float px,py,pz,vx,vy,vz,rho,prs,foam;
 * uint32 id, flags, pad; float ax,ay,az,pad (acc travels so that a migrant's 80-byte record is complete
 * on its new owner).  Buffers passed to pack/unpack are DEVICE pointers. */
#define SPH_SLAB_REC_BYTES 64
#define SPH_SLAB_OUT_BYTES 64
/* `ids` are global particle ids (they fix the summation order, so results do not depend on the
 * decomposition); `capacity` bounds owned + ghost + migrated-in slots. */
int sph_create_slab(SphEngine** out, const SphParticle* particles, const uint32_t* ids, size_t n,
                    const SphParams* params, int z0, int z1, int hasLo, int hasHi, size_t capacity, void* stream);
/* Classify by current position, emit records for the lower / upper neighbour (migrants + boundary
 * layer copies); countsOut = records written per direction.  Synchronises. */
int sph_slab_pack(SphEngine* e, void* sendLo, void* sendHi, uint32_t capLo, uint32_t capHi, uint32_t countsOut[2]);
/* Append the records received from the lower / upper neighbour. */
int sph_slab_unpack(SphEngine* e, const void* recvLo, uint32_t nLo, const void* recvHi, uint32_t nHi);
/* Owned particles as 64-byte records (pos3, vel3, acc3, rho, P, foam, uint32 id, flags, 2 pad) into host memory. */
int sph_slab_download(SphEngine* e, void* hostOut, size_t capRecords, size_t* nOut);

/* ---- the same exchange without host round trips, and its RCCL transport ------------------------------------------
 * The engine owns four device buffers (send lo / hi, receive lo / hi) of sph_slab_face_bytes(): a 64-byte header (magic, halo
 * copies, migrants, the sender's true counts, exchange number), then faceCap 64-byte records for MIGRANTS (the layout above),
 * then faceCap 40-byte records for HALO COPIES (float px,py,pz,vx,vy,vz,rho,prs; uint32 id, flags: what a neighbour candidate
 * needs -- round 4).  Counts never travel through the host.  Per substep a rank calls sph_slab_exchange
 * (pack -> per z-neighbour two grouped ncclSend / ncclRecv pairs over xGMI: header + migrants in use, halo copies in use ->
 * unpack, all on the engine's stream) and then sph_dispatch.  MESSAGE SIZES: the whole face, unless the face has been calm (its
 * record counts of the last two known exchanges within 3 % of each other, no impulse / container edit / re-priming in the last
 * three exchanges): then the records in use two exchanges ago + a quarter + 1024 (read back asynchronously into pinned memory,
 * so the path never waits for the device; both ends of a link derive the size from the same numbers: the sender from its own
 * counts, the receiver from the headers it received then).  A message that turns out too small sets SPH_SLAB_FLAG_TRUNCATED on the
 * receiver (records were cut off).
 * sph_slab_pack_async / sph_slab_unpack_async are the two halves for hosts that move the faces themselves (several slab
 * engines in one process, another transport): move sph_slab_face_bytes() bytes, or the three parts in use.  Overflows (send
 * face, slot capacity) set a device-side flag that sph_slab_status / sph_slab_download report.  faceCap must be the same on
 * all ranks of a communicator: the first sph_slab_exchange of an engine on a communicator checks that with one ncclAllReduce
 * (and one stream synchronisation) and fails instead of hanging.  A `stream` of NULL at creation means an engine-owned stream:
 * everything above is ordered on THAT stream.  While param_pause is set sph_slab_exchange and the step calls below do nothing
 * (as the paused DispatchCompute, SPHFluid3D.cpp:432): the halo records in place stay valid; all ranks must pause together. */
#define SPH_COMM_ID_BYTES 128
#define SPH_SLAB_HALO_BYTES 40
typedef struct SphComm SphComm;
int sph_slab_alloc_faces(SphEngine* e, uint32_t faceCap);
int sph_slab_face_buffer(SphEngine* e, int which /* 0 send lo, 1 send hi, 2 recv lo, 3 recv hi */, void** devPtr);
int sph_slab_face_bytes(SphEngine* e, uint64_t* bytes);
int sph_slab_pack_async(SphEngine* e);
int sph_slab_unpack_async(SphEngine* e, const void* recvLo, const void* recvHi, uint32_t recvCap);
/* The exchange's flags: device side, sticky until sph_slab_clear_flags, out[4] of sph_slab_status.  ERRORS -- records were lost;
 * sph_slab_status and sph_slab_download then return an error.  One NOTICE -- nothing lost, the calls succeed and out[4] carries the bit. */
enum {
    SPH_SLAB_FLAG_SEND_OVERFLOW = 1,    /* error: a send face overflowed */
    SPH_SLAB_FLAG_SLOT_OVERFLOW = 2,    /* error: the slot capacity overflowed while appending received records */
    SPH_SLAB_FLAG_BAD_HEADER = 4,       /* error: a received message did not start with a valid header */
    SPH_SLAB_FLAG_TRUNCATED = 8,        /* error: the neighbour had more records than its message carried */
    SPH_SLAB_FLAG_LAYER_JUMP = 16,      /* notice: a particle crossed MORE cell layers in z within one substep than the exchange follows */
    SPH_SLAB_FLAG_SIZE_MISMATCH = 32    /* error: the two ends of a link sized an exchange's messages differently (see the plans below) */
};
/* Synchronises; out = {records packed for lo, for hi, slots in use, -, flags (SPH_SLAB_FLAG_*)}.  SPH_SLAB_FLAG_LAYER_JUMP: the exchange
 * follows up to 3 layers per substep (the pack and the face launches of a boundary-first step cover the 5 lowest / highest
 * local layers; migrants go to the adjacent rank, which such a jump still reaches while every slab is at least 4 layers
 * thick); beyond that -- a particle placed far outside the container, a container that moved by cells under the fluid, a
 * slab thinner than the jump -- the decomposed run goes on but no longer equals the single-domain run, and says so here.
 * (SPHFluid.comp moves a particle with the uncapped velocity (v + a dt) dt, so this is a property of the scene, not a guarantee:
 * the BASELINE workloads stay far inside it through their whole collapse; the pack after a container change scans
 * every slot, so a change of shape alone is followed exactly as long as no particle has to cross a whole slab.) */
int sph_slab_status(SphEngine* e, uint32_t out[5]);
/* Clears the given flag bits (synchronises): a host acknowledges SPH_SLAB_FLAG_LAYER_JUMP and goes on. */
int sph_slab_clear_flags(SphEngine* e, uint32_t mask);
/* Bytes of the last exchange's messages to the lower / upper neighbour, and the bytes a whole face would be: {sent lo, sent hi,
 * face lo, face hi} (host-side bookkeeping, no synchronisation). */
int sph_slab_message_bytes(SphEngine* e, uint64_t out[4]);
/* Host-only (no device): the sizing rule itself -- records a message carries, given the face's record count two exchanges ago, three
 * exchanges ago, and the face capacity: the capacity unless the two counts are within 3 % + 64 of each other, else count + 25 % + 1024. */
int sph_slab_message_records(uint32_t seen, uint32_t before, uint32_t cap);
/* ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy: rank 0 creates the id and hands its 128 bytes to the other ranks
 * by any means (MPI, a file, torch.distributed); one rank per process, on the current HIP device. */
/* The nccl* entry points are loaded with dlopen ("librccl.so.1"); the environment variable SPH_RCCL_LIBRARY names another library to load them from.  The tests use
 * it to put a stand-in transport in RCCL's place that runs between processes on ONE GPU and refuses a receive whose size differs from its send's
 * (tests/fake_rccl/fake_rccl.c, tests/test_gpu_fake_rccl.py). */
int sph_comm_unique_id(void* out128);
int sph_comm_create(SphComm** out, const void* id128, int rank, int world);
int sph_comm_destroy(SphComm* comm);
/* Health check of the transport on this rank alone: one grouped ncclSend + ncclRecv of `bytes` bytes (a multiple of 4, at
 * most 2^30) from the rank to itself on a non-blocking stream, compared on the host.  Synchronises.  (The only way to
 * execute ncclSend / ncclRecv on a one-GPU box: RCCL refuses two ranks on one device.) */
int sph_comm_selftest(SphComm* comm, uint64_t bytes);
/* The same, also returning the hipEvent time of the grouped send + receive alone (ms). */
int sph_comm_selftest_timed(SphComm* comm, uint64_t bytes, float* msOut);
int sph_slab_exchange(SphEngine* e, SphComm* comm);

/* ---- agreement of the two ends of a link (round 5; no reference counterpart) -----------------------------------------
 * The sizes of an exchange's messages are derived on each rank by itself: the sender from its own record counts of two exchanges ago, the
 * receiver from the headers it received then, both from their own exchange number and from whether something stirred the fluid lately (an
 * impulse, a container / grid edit, a priming exchange: "hold", whole faces for three exchanges).  That only agrees while every rank makes the
 * same calls; ncclSend / ncclRecv with sizes that do not agree hang or cut records off.  So every sized exchange has a PLAN, 64 bytes: */
typedef struct SphSlabIntent {
    uint32_t magic;            /* "PLAN" */
    uint32_t exchangeNo;       /* sized exchanges this engine has enqueued before this one */
    uint32_t stepNo;           /* boundary-first steps begun */
    uint32_t faceCap;
    uint32_t sendHalo[2], sendMig[2];   /* records this engine's messages to the lower / upper neighbour carry */
    uint32_t recvHalo[2], recvMig[2];   /* records it posts receives for, from the lower / upper neighbour */
    uint32_t holdEvents;       /* impulses / container and grid edits / priming exchanges seen so far */
    uint32_t paramsHash;       /* FNV-1a of the SphParams the exchange is planned under */
    uint32_t flags;            /* 1 paused, 2 message test hook, 4 this exchange holds whole faces */
    uint32_t zRange;           /* z0 | z1 << 16: the cell layers this engine owns */
} SphSlabIntent;
/* ... and nothing moves before the plans of both ends of every link have been compared:
 *   - sph_slab_step_finish_local compares the neighbour ENGINES' plans directly;
 *   - sph_slab_exchange / sph_slab_step_finish send the plan across each link as a FIXED-SIZE message on a stream of its own, wait for the
 *     neighbours' plans on the host (polled, at most the deadline: SPH_ERR_TIMEOUT) and compare.  A difference is SPH_ERR_STATE on BOTH
 *     ranks of the link, with what differs by name ("this rank has seen 4 impulses ..., the upper neighbour 3"), before a sized message is
 *     posted.  Cost: one 64-byte send / receive per neighbour and exchange, and the host's look-ahead shrinks from two exchanges to about
 *     one (the device still holds more than a substep of queued work while the host waits).  sph_slab_set_verify(engine, 0) switches it
 *     off: then there is no host wait on the path beyond the pinned-memory read of counts that are two exchanges old, and agreement rests
 *     on the ranks' call sequences being the same.
 * Behind both there is a device-side check: a header names the sizes its sender's messages carry, the receiver's unpack compares them with the
 * sizes it received: SPH_SLAB_FLAG_SIZE_MISMATCH (an error of sph_slab_status / sph_slab_download). */
int sph_slab_set_verify(SphEngine* e, int mode /* 1 (default) | 0 */);
/* Limit of every host-side wait for a neighbour (default 30 s). */
int sph_slab_set_deadline(SphEngine* e, double seconds);
/* The plan of the last sized exchange, and (nullable) the host time its handshake waited, in ms. */
int sph_slab_plan(const SphEngine* e, SphSlabIntent* out, float* handshakeMsOut);
/* Host-only: 1 if `neighbour` (the plan of the engine on side 0 = below / 1 = above of `mine`) fits `mine`, else 0 and the reason in `why`. */
int sph_slab_plans_agree(const SphSlabIntent* mine, const SphSlabIntent* neighbour, int side, char* why, size_t whyBytes);
/* sph_sync that cannot hang: polls the engine's streams; SPH_ERR_TIMEOUT after `seconds` (<= 0: the engine's deadline) with where this engine stands. */
int sph_sync_deadline(SphEngine* e, double seconds);
/* Test hook (replaces round 4's environment variable): messages carry the count of two exchanges ago, no margin, no calm rule. */
int sph_slab_debug_tight_messages(SphEngine* e, int on);
/* The engine's exchange pattern on ONE rank, the rank being its own lower and upper neighbour: first the 64-byte plans (with the handshake's
 * polled wait), then the routine sph_slab_exchange itself posts the faces with -- per neighbour two ncclSend / ncclRecv pairs of UNEQUAL sizes
 * in one group: header + counts[2 + d] migrants, counts[d] halo copies -- over faces of capacity faceCap filled with a pattern; every byte is
 * compared (inside a message: arrived; beyond it: untouched).  msOut (nullable): hipEvent time of the faces' group. */
int sph_comm_selftest_faces(SphComm* comm, uint32_t faceCap, const uint32_t counts[4], float* msOut);
/* ---- boundary-first substep: the exchange hidden behind the interior of the SPH pass -----------------------------
 * sph_slab_step_begin = sph_dispatch, except that the SPH pass runs the slot ranges next to the slab's faces first (the
 * five lowest / five highest local cell layers: everything the next pack can touch as long as a substep moves a particle
 * across at most three layers; a substep that does not is reported, SPH_SLAB_FLAG_LAYER_JUMP above), and then, on a second stream of the engine, the pack of the exchange that prepares the
 * NEXT substep -- while the interior slots are still being computed on the engine's stream.  The second half moves the
 * faces and unpacks, still on the second stream; the engine's stream waits for it only at its end:
 *   sph_slab_step_finish(engine, comm)            one process per GPU: grouped ncclSend / ncclRecv (RCCL over xGMI)
 *   sph_slab_step_finish_local(engine, lo, hi)    several slab engines in ONE process: device-to-device copies of the
 *                                                 neighbours' send faces (call every engine's _begin before any _finish_local)
 * Both transports run the same stream / event schedule.  The state a step leaves behind already holds the halo records of
 * the next substep, so a run is: one plain exchange (sph_slab_exchange, or pack_async / unpack_async) to prime it, then
 * only steps; impulses go between steps as usual (they act on the halo copies as on their owners).  Members that move the
 * grid (box centre / half / angles, h, grid_cap) must not change between two steps: sph_slab_step_begin compares the grid with the
 * one the halo records in place were cut for and returns SPH_ERR_STATE (prime again with a plain exchange, then go on).  Every
 * engine of a group must begin a step before any of them finishes it (sph_slab_step_finish_local checks the neighbours' step
 * numbers).  Results are bit-identical to exchange + sph_dispatch. */
int sph_slab_step_begin(SphEngine* e, float overrideDt);
int sph_slab_step_finish(SphEngine* e, SphComm* comm);
int sph_slab_step_finish_local(SphEngine* e, SphEngine* lo, SphEngine* hi);
/* With SPH_OPT_TIMING on: hipEvent times of the LAST boundary-first step, in ms (synchronises): {pack, transfer, unpack} on the
 * exchange stream, then the end of the exchange and the end of the SPH pass (interior included), both measured from the start of
 * the step.  The transfer was hidden behind the interior iff out[3] <= out[4]. */
int sph_slab_step_times(SphEngine* e, float outMs[5]);

/* ---- measurement ----------------------------------------------------------------- */
enum {
    SPH_K_BIN = 0,      /* cell index + histogram   (BuildGrid.comp)            */
    SPH_K_SCAN = 1,     /* exclusive scan + clear   (ClearGrid.comp)            */
    SPH_K_SCATTER = 2,  /* counting-sort scatter + canonical rank               */
    SPH_K_SPH = 3,      /* 27-cell density+force+integrate+XSPH (+fused OBB)    */
    SPH_K_WRITEBACK = 4,/* 80-byte AoS update                                   */
    SPH_K_IMPULSE = 5,  /* WaveImpulse                                          */
    SPH_K_OTHER = 6,
    SPH_K_COUNT = 7
};
/* Accumulated hipEvent milliseconds and launch counts per kernel class since the
 * last reset (SPH_OPT_TIMING must be 1). Synchronises. */
int sph_kernel_times(SphEngine* e, double msOut[SPH_K_COUNT], int64_t launchesOut[SPH_K_COUNT], int reset);

/* ---- checkpoints: save, restore and digest the engine's state ------------------------------
 * A checkpoint is a blob of bytes from which another engine continues the run bit for bit: the records and the outputs of every
 * feature the blob carries are those of the uninterrupted run.  The digest is the checksum of a section computed on the device: two
 * engines whose digests agree hold the same state, and a blob proves on load that it is intact.
 *
 * The blob is little-endian.  All offsets are from the blob's first byte.
 *   header, 256 bytes
 *       0  uint64   magic "SPHSTATE" (0x4554415453485053)
 *       8  uint32   format version (SPH_STATE_FORMAT)          12  uint32  sph_abi_version() of the saving library
 *      16  uint32   checksum kind (SPH_STATE_CHECKSUM_MIX64)   20  uint32  number of sections
 *      24  uint64   n, the particle count                      32  uint64  total bytes of the blob
 *      40  uint32   mask of the sections present (SPH_STATE_*) 44  uint32  256, the header's size
 *      48  SphParams of the saved engine (132 bytes), then zeros up to byte 240
 *     240  2 x uint64  checksum of bytes [0, 240) and of the section table (word indices run on from the header into the table)
 *   section table at 256: per section 40 bytes
 *       0  uint32 tag (one SPH_STATE_* bit)   4  uint32 section version (1)   8  uint64 offset   16  uint64 bytes (a multiple of 8)
 *      24  2 x uint64 checksum of the payload (word index 0 at its first byte)
 *   payloads, in the table's order (ascending tags), each at the next multiple of 16 behind what lies before it, the gaps and the
 *   end of the blob (a multiple of 16) filled with zeros.  The layout is canonical: a blob with one byte changed anywhere is refused.
 *
 * The checksum of a byte range read as little-endian 64-bit words w_i (i from a base word index, 0 unless stated):
 *       lane L = sum over i of mix64(w_i + C_L + (base + i) * G) mod 2^64,  L = 0, 1
 *       mix64(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31   (splitmix64's finaliser)
 *       G = 0x9e3779b97f4a7c15, C_0 = 0x243f6a8885a308d3, C_1 = 0x13198a2e03707344
 * The terms are keyed by the word index (swapping two different records changes the sums) and the sums commute, so the checksum of a
 * concatenation is the sum of the pieces' checksums at their base indices.  It is an integrity check, not a cryptographic hash.
 *
 * Sections (the records are StateCore, StateTracers, StateDiffuse, StateScalars, StateObstacles, StateGates, StateMonitorSlot of csrc/sph_state.h):
 *   CORE       SphParams, lastDt, SphFountain (with the current seed), SphRiver, uint64 terrain count T, uint64 stencil count S; T floats of the
 *              heightfield (padded with zeros to 8 bytes); S float4 stencil targets
 *   PARTICLES  the n 80-byte records by particle id, exactly what sph_download_particles returns
 *   TRACERS    uint64 M, uint32 integrator, history K, stride, the three device words (substeps low / high, next ring slot), uint64 host
 *              mirror of the step counter c; M 32-byte records in the caller's order; the written slots of the pathline ring, min(c / stride + 1, K)
 *              x M float4 in slot order (a slot no snapshot has reached yet holds nothing a call returns, and is not saved)
 *   GATES      int32 count, uint32 history H, stride, words per books table A, words per ring row R, 0; SPH_MAX_GATES SphGate as set; A 8-byte
 *              words of the books (all gates' SphGateBooks, time, substeps, ring substeps); H x R words of the ring
 *   MONITORS   SPH_MAX_MONITORS slot records of 80 bytes (kind, 0, uint64 points M, dims, origin, spacing, the config in force, 0); then per slot
 *              that holds a monitor: substeps, acting substeps (uint64), time (double); M float4 points (explicit points only); M 128-byte
 *              rows; history x ringPoints 32-byte samples; history doubles
 *   DIFFUSE    SphDiffuseConfig, SphDiffuseCrest in force, uint32 crest on, crest books exist, state words W, crest words V, alive A, 0; W
 *              32-bit state words of the pool (alive, substep counter, class counts, totals; padded to 8 bytes); V crest words if the books
 *              exist (padded); the A living 48-byte records in pool order
 *   SCALARS    int32 K, uint32 table exists, bytes of the injected books B, the device word of the last diffusion number, uint64 substeps,
 *              8 floats D_k and lambda_k, 4 beta, 4 ref, int32 sources, 3 x 0, SPH_MAX_SCALAR_SOURCES SphScalarSource; n x K floats by
 *              particle id (padded to 8 bytes); B bytes of the books (sums, hits, time, substeps) if the table exists
 *   OBSTACLES  int32 bodies C, uint32 bytes of a device body record R, of a device dynamics record D, of the impulse sums S; 16 x int32 shape,
 *              dynamic, bound volume (-1: none); 16 SphObstacleDynamics as set; 16 x (dims[3], spacing[3]) per volume slot (dims 0: empty);
 *              C x R bytes of the bodies as they stand on the device (advanced poses); S bytes of the sums (C > 0); C x D bytes; per volume
 *              slot in use its dims[0] x dims[1] x dims[2] floats (padded to 8 bytes).  R, D and S must be this build's.
 * A section is present iff the saved engine held the feature (gates: at least one gate).  CORE and PARTICLES always are.
 *
 * NOT saved: query results (neighbour lists, components, kNN rows, ray hits and spans, shell, aniso, surface, statistics: derived; after a
 * load they are "no result", as after sph_reset); timing sums, debug counters and the graph cache (a load empties it); engine options
 * (they do not change bits; the loading engine keeps its own, so a blob saved under one pass variant, record mode or graph setting is
 * continued under another); the initial particles (after a load sph_initial_particles returns the loaded records, as after
 * sph_create_from_particles).  The processing orders (slot order, the tracers' and monitors' perm) are rebuilt: no output depends on them. */
#define SPH_STATE_FORMAT 1
#define SPH_STATE_CHECKSUM_MIX64 1
#define SPH_STATE_SECTION_COUNT 8
enum {
    SPH_STATE_CORE = 1, SPH_STATE_PARTICLES = 2, SPH_STATE_TRACERS = 4, SPH_STATE_DIFFUSE = 8, SPH_STATE_SCALARS = 16, SPH_STATE_OBSTACLES = 32,
    SPH_STATE_GATES = 64, SPH_STATE_MONITORS = 128
};
/* What sph_state_peek reads from a blob; section with tag 1 << i is at index i (bytes 0: absent). */
typedef struct SphStateInfo {
    uint32_t formatVersion, abiVersion, checksumKind, sections;
    uint64_t n, totalBytes;
    SphParams params;
    uint32_t pad;
    uint32_t version[SPH_STATE_SECTION_COUNT];
    uint64_t offset[SPH_STATE_SECTION_COUNT], bytes[SPH_STATE_SECTION_COUNT];
    uint64_t sum[SPH_STATE_SECTION_COUNT][2];
    uint64_t terrainCount, terrainOffset;   /* of the core section: the heightfield's floats and where they lie in the blob (count 0: none) */
    uint64_t stencilCount;                  /* the stencil targets it carries */
} SphStateInfo;
/* The digests of a live engine: sum[i] is the checksum a blob saved now would store for the section with tag 1 << i. */
typedef struct SphStateDigest {
    uint32_t sections;                 /* the sections digested (those asked for that the engine holds) */
    uint32_t pad;
    uint64_t sum[SPH_STATE_SECTION_COUNT][2];
} SphStateDigest;

/* The bytes sph_state_save would write now. */
int sph_state_size(SphEngine* e, size_t* bytes);
/* Writes the blob.  Synchronises; brings the 80-byte records up to date as sph_download_particles does and changes nothing else a later
 * dispatch reads: a run with saves gives the bytes of the run without.  cap too small: SPH_ERR_CAPACITY, *written holds the need.
 * SPH_ERR_STATE on a z-slab engine. */
int sph_state_save(SphEngine* e, void* blob, size_t cap, size_t* written);
/* Makes the engine what the saved one was, whatever it held before (another n, other features, junk books): the sph_reset path for the
 * particles, every feature's own set path for its buffers, then the saved buffers and counters over what the set calls zeroed.  Features
 * the blob does not carry are cleared (obstacles and volumes too).  A volume comes back in the slot it had.  Synchronises.
 * Everything is validated BEFORE the engine is touched -- the blob as by sph_state_peek, then the params and every feature's config by
 * the checks of the set calls: a bad blob is SPH_ERR_ARG with a message that names what is wrong, and the engine is bit for bit what it
 * was (sph_state_digest proves it).  SPH_ERR_STATE on a z-slab engine, and under SPH_OPT_GRID_BUILD 1 for a blob with feature sections,
 * before anything is touched.  Only a failing HIP call (an allocation, say) can stop a load halfway: the engine is then valid and
 * destroyable, it holds the blob's core state and particles if those were reached, the features restored before the failure, and none
 * of the others; load again or sph_reset. */
int sph_state_load(SphEngine* e, const void* blob, size_t bytes);
/* Host only, no device: validates the whole blob (magic, versions, layout, every size against its own config, every checksum) and
 * reports its header and section table. */
int sph_state_peek(const void* blob, size_t bytes, SphStateInfo* out);
/* The checksums of the engine's sections computed on the device (sections: a mask of SPH_STATE_*, 0 = all the engine holds): no array
 * moves to the host, one read of 16 bytes per section.  What is read first, because a size or a count lies there: the pool's state and
 * crest words (112 bytes), the scalars' diffusion word, and the last 32-bit word of an array with an odd number of them.  By definition
 * what a blob saved at this moment stores (sph_state_peek's sum).  Brings the records up to date like sph_state_save.  Synchronises. */
int sph_state_digest(SphEngine* e, uint32_t sections, SphStateDigest* out);
/* Host only: the checksum above of n bytes (n % 8 == 0) at base word index 0. */
int sph_state_checksum_host(const void* bytes, size_t n, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* SPH_ABI_H */
