// sph_engine.hip -- host driver + C-ABI of the MI355X SPH substep engine.
//
// Replaces the GL compute dispatch path of SPHFluidGPU
// (/root/reference/ComponentFramework/SPHFluid3D.cpp:431-522 DispatchCompute, :604-623
// ApplyWaveImpulse, :713-731 ResetSimulation, :32-83 ctor/dtor) behind include/sph_abi.h.
// No CPU fallback: every compute entry point fails with SPH_ERR_HIP when HIP does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sph_abi.h"
#include "sph_host.h"
#include "sph_kernels.h"
#include "sph_walk.h"
#include "sph_sample.h"
#include "sph_neighbors.h"
#include "sph_components.h"
#include "sph_knn.h"
#include "sph_aggregate.h"
#include "sph_conv.h"
#include "sph_posgrad.h"
#include "sph_convgrad.h"
#include "sph_shell.h"
#include "sph_aniso.h"
#include "sph_rays.h"
#include "sph_surface.h"
#include "sph_tracer.h"
#include "sph_diffuse.h"
#include "sph_scalar.h"
#include "sph_obstacle.h"
#include "sph_volume.h"
#include "sph_stats.h"
#include "sph_couple.h"
#include "sph_gate.h"
#include "sph_monitor.h"
#include "sph_state.h"

static_assert(sizeof(SphParticle) == 80, "SPHParticle must be 80 bytes (SPHFluid3D.h:12-24)");
static_assert(sizeof(SphSample) == 32, "SphSample must be 32 bytes");
static_assert(sizeof(SphTracer) == 32, "SphTracer must be 32 bytes");
static_assert(sizeof(SphDiffuse) == 48 && sizeof(sph::DiffuseRec) == 48 && sizeof(SphDiffuseConfig) == 64 && sizeof(SphDiffuseInfo) == 88, "SphDiffuse must be 48 bytes, SphDiffuseConfig 64, SphDiffuseInfo 88");
static_assert(SPH_DIFFUSE_SPRAY == sph::DF_SPRAY && SPH_DIFFUSE_FOAM == sph::DF_FOAM && SPH_DIFFUSE_BUBBLE == sph::DF_BUBBLE, "diffuse classes of sph_abi.h and sph_diffuse.h");
static_assert(sizeof(SphScalarMoments) == 40, "SphScalarMoments must be 40 bytes");
static_assert(SPH_MAX_SCALAR_CHANNELS == sph::kScalarMax && SPH_SCALAR_SET == sph::kScalarSet && SPH_SCALAR_ADD == sph::kScalarAdd, "scalar constants of sph_abi.h and sph_scalar.h");
static_assert(sizeof(SphScalarSource) == sizeof(sph::CoupleSrc) && SPH_MAX_SCALAR_SOURCES == sph::kCoupleMax && SPH_SOURCE_SPHERE == sph::COUPLE_SPHERE &&
              SPH_SOURCE_BOX == sph::COUPLE_BOX && SPH_SOURCE_RATE == sph::COUPLE_RATE && SPH_SOURCE_RELAX == sph::COUPLE_RELAX, "SphScalarSource must be 64 bytes");
static_assert(sizeof(SphGate) == sizeof(sph::GateRec) && sizeof(SphGateBooks) == 8 * sph::kGateWords && SPH_MAX_GATES == sph::kGateMax &&
              SPH_MAX_GATE_HISTORY == sph::kGateHistoryMax && SPH_GATE_RECT == sph::GATE_RECT && SPH_GATE_ELLIPSE == sph::GATE_ELLIPSE &&
              SPH_GATE_UNBOUNDED == sph::GATE_UNBOUNDED && SPH_MAX_SCALAR_CHANNELS == sph::kGateChannels, "SphGate must be 64 bytes, SphGateBooks 72");
static_assert(sizeof(SphMonitorRow) == sizeof(sph::MonitorRow) && offsetof(SphMonitorRow, sumVelVel) == offsetof(sph::MonitorRow, sumVelVel) &&
              sizeof(SphMonitorConfig) == 24 && sizeof(SphMonitorInfo) == 112 && SPH_MAX_MONITORS == sph::kMonitorMax && SPH_MONITOR_TKE == sph::kMonTke &&
              SPH_MONITOR_WET_SHARE == sph::kMonWetShare && SPH_MONITOR_VAR_PRESSURE == sph::kMonVarPressure, "SphMonitorRow must be 128 bytes");
static_assert(sizeof(SphObstacle) == 76 && SPH_MAX_OBSTACLES == sph::kObsMax, "SphObstacle must be 76 bytes");
static_assert(sizeof(SphObstacleDynamics) == 80, "SphObstacleDynamics must be 80 bytes");
static_assert(SPH_MAX_VOLUMES == sph::kVolMax && SPH_MAX_OBSTACLES == sph::kVolBodies && sizeof(SphVolumeHost) == 32, "SphVolumeHost must be 32 bytes");
static_assert(sizeof(SphSurfaceVertex) == 24 && sizeof(sph::SurfVertex) == 24, "SphSurfaceVertex must be 24 bytes");
static_assert(sizeof(SphStatistics) == 832 && alignof(SphStatistics) == 8 && sizeof(SphHistogramSpec) == 16, "SphStatistics must be 832 bytes, SphHistogramSpec 16");

struct SphEngine;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(SPH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

template <class T>
int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return SPH_OK;
}
template <class T>
void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

// An engine-owned device scratch array that only grows.  No destructor: frees stay explicit, behind the stream drains they follow.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                                  // elements
    int grow(SphEngine* e, size_t need);             // to at least `need` elements; contents are not kept, the engine's stream is drained first
    void release() { dev_free(p); cap = 0; }
};

// Pinned staging for stream-ordered uploads: kObsSlots slots of `per` records, each guarded by an event recorded behind the copy queued from it.
constexpr int kObsSlots = 4;
template <class T>
struct StageRing {
    T* h = nullptr;
    hipEvent_t ev[kObsSlots] = {nullptr, nullptr, nullptr, nullptr};
    size_t per = 0;
    int cur = 0;                                     // the slot handed out last
    hipError_t create(hipStream_t stream, size_t perSlot) {
        per = perSlot;
        hipError_t er = hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(T) * per * kObsSlots, hipHostMallocDefault);
        for (auto& v : ev) if (er == hipSuccess) er = hipEventCreateWithFlags(&v, hipEventDisableTiming);
        for (auto& v : ev) if (er == hipSuccess) er = hipEventRecord(v, stream);      // (so that the first wait for a slot succeeds)
        return er;
    }
    // The next slot, once the copy queued from it last time has run.
    int next(T** slot) {
        cur = (cur + 1) % kObsSlots;
        HIP_TRY(hipEventSynchronize(ev[cur]));
        *slot = h + (size_t)cur * per;
        return SPH_OK;
    }
    // Behind the copy queued from the slot just handed out.
    int commit(hipStream_t stream) {
        HIP_TRY(hipEventRecord(ev[cur], stream));
        return SPH_OK;
    }
    void destroy() {
        if (h) (void)hipHostFree(h);
        h = nullptr;
        for (auto& v : ev) { if (v) (void)hipEventDestroy(v); v = nullptr; }
        cur = 0;
    }
};

// Records the kernels read from device memory (a replayed graph sees a later upload), with the pinned staging of their stream-ordered
// uploads.  No destructor, like DevBuf.
template <class T>
struct DevTable {
    T* p = nullptr;
    StageRing<T> stage;                              // `count` records per slot
    // The first call makes `count` records and the staging; a failure leaves nothing behind (`what` names the staging in its message).
    int ensure(SphEngine* e, size_t count, const char* what);
    int slot(T** out) { return stage.next(out); }    // the next pinned slot, to be filled in place and sent
    int send(SphEngine* e, size_t n = 1, size_t at = 0) { return send_part(e, 0, n * sizeof(T), at); }   // the slot's first n records to records at ..
    int send_part(SphEngine* e, size_t off, size_t bytes, size_t at);   // `bytes` at byte `off` of the slot's first record to the same bytes of record `at`
    int put(SphEngine* e, const T* src, size_t n = 1, size_t at = 0) {  // n finished records through the next slot
        T* s = nullptr;
        const int rc = slot(&s);
        if (rc) return rc;
        std::memcpy(s, src, n * sizeof(T));
        return send(e, n, at);
    }
    void release() { dev_free(p); stage.destroy(); }
};

inline int blocks_for(size_t n, int per = sph::kBlock) { return (int)((n + per - 1) / per); }

// The scratch of one 64-bit scan (scan_counts64_launch) of `rows` counts: blocks_for(rows, kScanTile) + 2 words of tile sums (the totals,
// sum and largest count, lie behind them) and one maximum per tile.  Dead once a scan's totals have been read.
struct ScanScratch {
    DevBuf<unsigned long long> tileSums;
    DevBuf<uint32_t> tileMax;
    int grow(SphEngine* e, size_t rows) {
        const size_t tiles = (size_t)blocks_for(rows, sph::kScanTile);
        const int rc = tileSums.grow(e, tiles + 2);
        return rc ? rc : tileMax.grow(e, tiles);
    }
    void release() { tileSums.release(); tileMax.release(); }
};

// One field monitor (sph_monitor.h): the table the kernels read with the table as uploaded last, the points and
// their processing order (explicit points only), the rows, the ring of history x ringPoints samples (two float4 each) and its history
// times.  Buffers only grow while the slot lives.
struct MonitorSlot {
    int kind = SPH_MONITOR_NONE;
    size_t m = 0;
    int dims[3] = {0, 0, 0};
    float origin[3] = {0.0f, 0.0f, 0.0f}, spacing[3] = {0.0f, 0.0f, 0.0f};
    SphMonitorConfig cfg{};
    DevTable<sph::MonitorTab> d_tab;
    sph::MonitorTab tab{};
    DevBuf<float4> d_points, d_ring;
    DevBuf<uint32_t> d_perm;
    DevBuf<sph::MonitorRow> d_rows;
    DevBuf<double> d_times;
};

}  // namespace

static std::set<SphEngine*> g_engines;      // live engines of this process (sph_destroy clears what neighbours hold of a destroyed one)
static std::mutex g_enginesMutex;           // (a host may drive its engines from one thread each)

// One exchange's true record counts as both ends of its links know them: what this engine packed (its Last* counter words) and what the
// headers it received named (nHaloTrue / nMigTrue of the face from direction d).  slab_note_counts writes, slab_plan reads.
struct SlabSeen { sph::SlabMsg sent, received; };
// The plans of one handshake: this engine's, and the ones received from the lower / upper neighbour.
struct SlabPlans { SphSlabIntent mine, from[2]; };
static_assert(sizeof(SphSlabIntent) == 64 && sizeof(SlabPlans) == 192, "a plan is a fixed 64-byte message");
static_assert(SPH_SLAB_FLAG_SEND_OVERFLOW == sph::kSlabFlagSendOverflow && SPH_SLAB_FLAG_SLOT_OVERFLOW == sph::kSlabFlagSlotOverflow && SPH_SLAB_FLAG_BAD_HEADER == sph::kSlabFlagBadHeader &&
              SPH_SLAB_FLAG_TRUNCATED == sph::kSlabFlagTruncated && SPH_SLAB_FLAG_LAYER_JUMP == sph::kSlabFlagLayerJump && SPH_SLAB_FLAG_SIZE_MISMATCH == sph::kSlabFlagSizeMismatch, "sph_device.h mirrors SPH_SLAB_FLAG_*");
static_assert(sizeof(sph::SlabRec) == SPH_SLAB_REC_BYTES && sizeof(sph::HaloRec) == SPH_SLAB_HALO_BYTES && sizeof(sph::SlabOut) == SPH_SLAB_OUT_BYTES, "the wire records of sph_slab.h have the sizes sph_abi.h names");

struct SphEngine {
    hipStream_t stream = nullptr;
    bool ownStream = false;
    SphParams params{};
    SphGridInfo grid{};
    size_t n = 0;
    size_t cap = 0;
    int allocatedCells = 0;
    uint32_t idBase = 0;

    // options
    int optNeighbor = 3, optGridBuild = 0, optAos = 1, optTiming = 0, optGraph = 0;   // optAos: 1 = records materialised on demand (default)
    // hipGraph cache of sph_dispatch_n (SPH_OPT_GRAPH): one executable graph per distinct call
    struct GraphEntry {
        uint64_t key = 0;
        std::vector<unsigned char> material;   // full key material, compared on a hit
        hipGraphExec_t exec = nullptr;
        int postCur = 0;
        bool postAos = false, postAcc = false;
        uint64_t lastUse = 0;
    };
    std::vector<GraphEntry> graphs;
    uint64_t graphClock = 0, graphLaunches = 0, graphCaptures = 0;

    // public contract buffer
    SphParticle* d_aos = nullptr;
    // internal sorted SoA state, double buffered
    float4* d_pos[2] = {nullptr, nullptr};
    float4* d_vel[2] = {nullptr, nullptr};
    float2* d_rp[2] = {nullptr, nullptr};
    float* d_foam[2] = {nullptr, nullptr};
    float4* d_acc = nullptr;
    int cur = 0;
    bool internalValid = false, aosValid = false, accValid = false;
    // grid / sort scratch
    uint2* d_binKey = nullptr;              // k_bin: (cell, arrival slot inside the cell) of every state slot
    uint32_t* d_order = nullptr;
    float4* d_stencil = nullptr;            // SetStencilTargets points (binding 5 of StencilAttract.comp)
    size_t stencilCount = 0;
    int32_t *d_llNext = nullptr, *d_llCell = nullptr, *d_llKey = nullptr;   // linked-list A/B variant (particleNext, particleCell, cellKey)
    uint2* d_tmp = nullptr;
    uint32_t *d_cellCount = nullptr, *d_cellStart = nullptr, *d_blockSums = nullptr;
    int32_t* d_dbg = nullptr;
    size_t dbgCap = 0;
    // z-slab (multi-GPU) mode: this engine owns global cell layers [z0, z1) and keeps one ghost layer per side
    bool slab = false;
    int z0 = 0, z1 = 0, hasLo = 0, hasHi = 0;
    size_t nSlots = 0;                      // state slots in use (live + dead), upper bound of the live count (= cap once the async exchange is used)
    char* d_face[4] = {nullptr, nullptr, nullptr, nullptr};   // engine-owned halo buffers: send lo / hi, recv lo / hi (sph::slab_face_bytes(faceCap): header, migrants, halo copies)
    // message sizing: the two messages per direction carry the records in use, sized from the counts of TWO exchanges ago
    // (read back asynchronously into pinned memory; both ends of a link see the same numbers: the sender its own count, the receiver the
    // header it got), the face capacity until those exist
    SlabSeen* h_seen = nullptr;             // pinned ring of 4 exchanges: the true counts this engine packed and the ones its neighbours' headers named
    hipEvent_t evCnt[4] = {nullptr, nullptr, nullptr, nullptr};
    bool cntValid[4] = {false, false, false, false};
    uint32_t exchangeNo = 0;                // sized exchanges enqueued so far
    sph::SlabMsg msgSend{}, msgRecv{};      // records the messages of the exchange being enqueued carry
    uint64_t sentBytes[2] = {0, 0};         // bytes of the last exchange's messages to lo / hi
    int calmHold = 0;                       // exchanges that still send whole faces because something just changed under the fluid (impulse, container, re-prime)
    uint32_t stepNo = 0;                    // boundary-first steps begun
    // the PLAN of an exchange and its agreement with the neighbours' plans (slab_plan, slab_intent_mismatch, slab_handshake_rccl)
    SphSlabIntent intent{};                 // what this engine is about to do in exchange intent.exchangeNo: compared with the neighbours' plans before a sized message is posted
    bool intentValid = false;
    uint32_t holdEvents = 0;                // things that set calmHold so far (impulses, container / grid edits, priming exchanges): every rank must have seen the same ones
    int verifyMode = 1;                     // RCCL transport: 1 (default) = the plans cross each link as a fixed 64-byte message and are compared BEFORE the sized messages are posted
    double deadlineSec = 30.0;              // host-side limit of a wait for a neighbour (handshake) and of sph_sync_deadline's default
    float lastDt = 0.0f;                    // dt of the last unpaused dispatch (0: none yet)
    int tightMessages = 0;                  // test hook (sph_slab_debug_tight_messages): the count of two exchanges ago, no margin, no calm rule
    hipStream_t hstream = nullptr;          // the handshake's stream
    hipEvent_t evIntent = nullptr;
    SlabPlans *d_intent = nullptr, *h_intent = nullptr;   // device / pinned host: the plans of one handshake
    float handshakeMs = 0.0f;               // host time the last handshake waited for its neighbours
    uint64_t handshakes = 0;
    bool stepPaused = false;                // the pending step is a paused one (nothing was enqueued)
    float packGrid[8] = {0};                // grid (gridMin, cellSize, dims) the halo records in place were cut for
    bool packGridValid = false;
    hipEvent_t evX[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // SPH_OPT_TIMING: pass start, pack start, pack end, transfer end, unpack end of the last step
    hipEvent_t evPassEnd = nullptr;         // SPH_OPT_TIMING: end of the SPH pass (interior included) of the last boundary-first step
    uint32_t faceCap = 0;
    const void* faceAgreedWith = nullptr;   // communicator whose ranks were checked to share faceCap (sph_slab_exchange)
    SphFountain fountain{};                 // fountain* members (SPHFluid3D.h:161-168)
    SphRiver river{};                       // river / terrain members (SPHFluid3D.h:171-196)
    std::vector<float> terrainHeights;      // CPU copy of the heightfield (:175); empty = river step off (:512)
    float* d_terrain = nullptr;             // terrainSSBO (binding 7 of TerrainConstraints.comp)
    size_t terrainCap = 0;
    float4 *d_sPV = nullptr, *d_sOwn = nullptr;   // sorted copy of the entry state: 32-byte records (pos, 1/rho | vel, P) + own data
    size_t sortedCap = 0;
    float4* d_shapeTab = nullptr;           // sampled curve of container shapes 9/11/12/14 (128 points)
    float shapeKey[8] = {-1.0f};            // parameters the uploaded table was built from
    sph::ShapeTab shapeTab{};
    // boundary-first substep (sph_slab_step_*): the halo exchange of the NEXT substep runs on xstream beside the interior of the SPH pass
    hipStream_t xstream = nullptr;
    hipStream_t bstream = nullptr;          // LOW priority: the interior launch of the SPH pass, beside the face launches on the engine's stream and the exchange on xstream
    hipEvent_t evBoundary = nullptr, evPacked = nullptr, evDone = nullptr, evSorted = nullptr, evInterior = nullptr;
    hipEvent_t peerDone[2] = {nullptr, nullptr};   // evDone of the lower / upper neighbour ENGINE of the last local transfer: it has read this engine's send face
    bool stepPending = false;               // sph_slab_step_begin ran, its finish has not yet
    bool slabOrderValid = false;            // slots are in the order of the last counting sort and no particle can have moved by more than a layer since
    float lastContainer[15] = {0};          // container / grid members of the last dispatch (a change may move particles by many cells, or the grid under them)
    uint32_t* d_slabCnt = nullptr;          // sph::kSlabCounters words, named by sph::SlabCounter (sph_slab.h)
    int debugFlags = 0;
    unsigned long long* d_stats = nullptr;   // k_sph_walk / k_sph_list diagnostics (SPH_OPT_DEBUG bit 3), see sph_debug_counters
    // sph_sample_points (host arrays): device copies of the probes and of the results
    DevBuf<float4> d_sampleIn;
    DevBuf<SphSample> d_sampleOut;
    // the queries that walk the grid by particle id (neighbour lists, kNN): ids of the sorted slots, refilled by every run (slot_ids_fill)
    DevBuf<int32_t> d_slotIds;
    // the scratch of the 64-bit scan of neighbour lists, components and shell
    ScanScratch scanScratch;
    // sph_neighbors_*: counts, the offsets of their scan, and the lists themselves (CSR)
    DevBuf<int32_t> d_nbIndices;
    DevBuf<uint32_t> d_nbCnt;
    DevBuf<long long> d_nbOffsets;
    SphNeighborInfo nbInfo{};               // kind 0: no lists
    bool nbIndexed = false;                 // d_nbIndices holds nbInfo.total entries
    // sph_components_*: per sorted slot the particle id, the union-find parent and the tree's smallest id; per particle id labels, roots and the
    // root flags with their scan (offsets); the table; the words of the launches (changed / more) and the table's reduction
    DevBuf<int32_t> d_ccIds, d_ccLabels, d_ccRoots;
    DevBuf<uint32_t> d_ccParent, d_ccMinId, d_ccFlag, d_ccWords;
    DevBuf<unsigned long long> d_ccStats;
    DevBuf<long long> d_ccOffsets;
    DevBuf<sph::CcRow> d_ccTable;
    SphComponentInfo ccInfo{};
    bool ccValid = false;                   // the buffers hold the result ccInfo describes
    int optCcVariant = 0;                   // SPH_OPT_COMPONENTS_VARIANT
    // sph_knn_*: the dense rows (indices, dist2: rows * k each), the counts and the two words of the reduction
    DevBuf<int32_t> d_knnIndices;
    DevBuf<float> d_knnDist2;
    DevBuf<uint32_t> d_knnCounts;
    DevBuf<unsigned long long> d_knnStats;
    SphKnnInfo knnInfo{};                   // kind 0: no rows
    // sph_rays_*: the staged rays of sph_rays_cast (two float4 each), the hits (two float4 each) and the two words of the reduction
    DevBuf<float4> d_rayIn, d_rayHits;
    DevBuf<unsigned long long> d_rayStats;
    DevBuf<uint2> d_rayBin;                 // the ordering of the rays by their cell of entry: (cell, arrival number) per ray, the histogram over
    DevBuf<uint32_t> d_rayCount, d_rayStart, d_rayBlockSums, d_rayOrder;   // numCells + 1 bins, its scan, the tile sums, the order
    int optRaysVariant = 0;                 // SPH_OPT_RAYS_VARIANT: 0 = rays cast in the caller's order, 1 = in the order of their cell of entry (same bits)
    SphRaysInfo raysInfo{};
    bool raysValid = false;
    // sph_rays_span*: the spans (two uint4 each) and the four words of their reduction; the staged rays and the ordering are the cast's scratch
    DevBuf<uint4> d_spanRows;
    DevBuf<unsigned long long> d_spanStats;
    int optRaySpansVariant = 0;             // SPH_OPT_RAY_SPANS_VARIANT: 0 = the layer walk, 1 = the block walk (same bits)
    SphRaySpansInfo spansInfo{};
    bool spansValid = false;
    int optKnnVariant = 0;                  // SPH_OPT_KNN_VARIANT: 0 = k_knn (LDS), 1 = k_knn_select (same bits)
    // sph_aggregate_*: the caller's values in slot order (the stage of the default variant); no result is kept
    DevBuf<float> d_aggStage, d_aggIn, d_aggOut;   // (d_aggIn / d_aggOut / d_aggCnt: the device side of sph_aggregate_staged's host arrays)
    DevBuf<uint32_t> d_aggCnt;
    // sph_aggregate_adjoint_* / _route_*: the counting sort of the query points (key, count, tile sums, start, arrival order, perm, sorted
    // points), arg in row order, and the device side of the staged call's g
    DevBuf<uint2> d_adjKey;
    DevBuf<uint32_t> d_adjCount, d_adjSums, d_adjStart, d_adjTmp, d_adjPerm, d_adjArg;
    DevBuf<float4> d_adjPts;
    DevBuf<float> d_adjIn;
    DevBuf<float> d_posStage;               // sph_aggregate_posgrad_*: g in slot order (particle targets) or in binned order (query targets)
    int optAggVariant = 0;                  // SPH_OPT_AGGREGATE_VARIANT: bit 0 gather by id (no stage), bits 1-2 channels per pass, bit 3 4-byte loads (same bits)
    // sph_shell_*: the rows by particle id (or by query point) and the ids of the shell; per sorted slot the normal with the shell flag and the
    // compacted shell slots of pass 2; the flag words by row and by slot with their scan (offsets); the two words of the reduction
    DevBuf<sph::ShellRow> d_shRows;
    DevBuf<int32_t> d_shIds, d_shSlots;
    DevBuf<float4> d_shNrm;
    DevBuf<uint32_t> d_shFlagRow, d_shFlagSlot;
    DevBuf<unsigned long long> d_shStats;
    DevBuf<long long> d_shOffsets;
    SphShellInfo shellInfo{};               // kind 0: no rows
    // sph_aniso_*: the rows by particle id, per sorted slot the three float4 a lattice node reads, the four words of the reduction
    DevBuf<sph::AnisoRow> d_anRows;
    DevBuf<float4> d_anSlots;
    DevBuf<unsigned long long> d_anStats;
    SphAnisoInfo anisoInfo{};               // kind 0: no rows
    int optShellTimed = 0;                  // SPH_OPT_SHELL_TIMED: which launches of a build the timing bracket covers (0 all, 1 pass 1, 2 pass 2, 3 scans and compactions)
    // sph_extract_surface*: scratch per lattice point (sampled volume, codes, vertex offsets) and per tile, and the borrowed outputs
    DevBuf<float> d_surfVol;
    DevBuf<uint16_t> d_surfCode;
    DevBuf<uint32_t> d_surfVOff, d_surfTris;
    DevBuf<uint2> d_surfTile;
    DevBuf<unsigned long long> d_surfTileOff;
    DevBuf<sph::SurfVertex> d_surfVerts;
    bool surfValid = false;
    uint32_t surfNumV = 0, surfNumT = 0;
    // sph_statistics*: per-tile sums / partial records / histogram rows, the cells kernel's rows, and the device copy of the host variant's result
    DevBuf<double> d_statSums;
    DevBuf<uint32_t> d_statPart, d_statHist;
    DevBuf<unsigned long long> d_statCell, d_statOut;

    // sph_tracers_*: M records in the caller's order (two float4 each), their processing order, the pathline ring of K x M float4, the
    // device step counter (sph_tracer.h) and the scratch of the processing order's cell sort
    float4* d_trRec = nullptr;
    uint32_t* d_trPerm = nullptr;
    float4* d_trRing = nullptr;
    uint32_t* d_trState = nullptr;
    uint2* d_trKey = nullptr;
    DevBuf<uint32_t> d_trCellCount, d_trCellStart, d_trBlockSums;
    size_t trM = 0, trCap = 0, trRingCap = 0;
    int trIntegrator = 0;
    uint32_t trK = 0, trS = 1;
    uint64_t trSteps = 0;                // host mirror of the device step counter: non-paused substeps issued since sph_tracers_set
    uint64_t trSorted = 0;               // trSteps at the last cell sort of the processing order
    bool trOrdered = false;              // the processing order has been cell-sorted since sph_tracers_set
    bool capturing = false;              // sph_dispatch_n is capturing its launches into a graph

    // sph_diffuse_* (sph_diffuse.h): the pool of C records (three float4 each) and the scratch pool a substep advances
    // into, the device state words (alive count, substep counter, totals), the coefficients as the kernels read them, the survivor flags
    // with their scan, the per-block counts, and the child counts in id order with their scan
    float4* d_dfPool = nullptr;
    float4* d_dfScratch = nullptr;
    uint32_t* d_dfState = nullptr;
    DevTable<sph::DiffuseCoef> d_dfCoef;
    uint32_t *d_dfFlag = nullptr, *d_dfFlagStart = nullptr, *d_dfFlagSums = nullptr, *d_dfPart = nullptr;
    DevBuf<uint32_t> d_dfCnt, d_dfCntStart, d_dfCntSums;
    uint32_t dfC = 0;                    // capacity of the pool (0: none)
    int optNbFill = 0;                   // SPH_OPT_NEIGHBORS_FILL: 0 = lane-owned stores (k_neighbors_fill), 1 = the wave-cooperative row write (same bits)
    int optDiffuseTimed = 0;             // SPH_OPT_DIFFUSE_TIMED: which launches of the substep the timing bracket covers (0 all, 1 advance, 2 the rest)
    SphDiffuseConfig dfCfg{};            // the config in force
    // crest births of the pool (sph_diffuse_set_crest): the coefficients and the books in device memory (made by the first set, kept as
    // long as the pool), and the scratch of the shell pass by slot, all its own (a captured graph bakes the
    // addresses in, and the scratch of sph_shell_* may be re-made by any query): normal and member word, 0 / 1 flag, its scan with the
    // tile scratch, the compacted shell slots, the crest per slot, the per-block rows of crest children
    DevTable<sph::DiffuseCrestCoef> d_dfCrCoef;
    uint32_t* d_dfCrState = nullptr;
    DevBuf<float4> d_dfCrNrm;
    DevBuf<uint32_t> d_dfCrFlag, d_dfCrPart;
    DevBuf<long long> d_dfCrOffsets;
    ScanScratch dfCrScan;
    DevBuf<int32_t> d_dfCrSlots;
    DevBuf<float> d_dfCrCrest;
    bool dfCrOn = false;
    SphDiffuseCrest dfCrCfg{};           // the crest config in force (all zero while off)

    // sph_scalars_* (sph_scalar.h): K channels per particle in the caller's order, their gathered copy in slot order
    // (K values + the ghost weight per slot), the coefficients as the kernels read them, and the device word of the last substep's
    // diffusion number
    float* d_scVal = nullptr;
    float* d_scSorted = nullptr;
    DevTable<sph::ScalarCoef> d_scCoef;
    uint32_t* d_scState = nullptr;
    int scK = 0;
    size_t scN = 0;                      // particles the buffers were allocated for
    float scCoeffs[2 * sph::kScalarMax] = {0};   // D_0 .. D_{K-1}, lambda_0 .. lambda_{K-1} as set
    uint64_t scSteps = 0;                // non-paused substeps issued since sph_scalars_set
    int optScalarSweep = 0;              // SPH_OPT_SCALAR_SWEEP: 0 = plain walk, 1 = LDS-staged
    DevBuf<float4> d_scView;             // sph_scalars_moments: a channel laid out as the statistics kernels' input (3 float4 per slot)
    DevBuf<float2> d_scViewRp;
    DevBuf<float> d_scSampleOut;         // sph_scalars_sample_points (host arrays): device copy of the results
    // sph_scalars_set_buoyancy / _set_sources (sph_couple.h): the table the kernel reads with its host mirror, the
    // books, and the per-block partial rows.  They belong to the scalar set: allocated by the first call that switches something on,
    // freed with the channels.
    DevTable<sph::CoupleTab> d_cpTab;
    sph::CoupleAcc* d_cpAcc = nullptr;
    double* d_cpPart = nullptr;
    sph::CoupleTab cpTab{};              // host mirror of *d_cpTab.p
    bool cpBuoy = false;                 // a beta is non-zero: the kick runs, and the pass does not keep the 80-byte array current

    // sph_gates_* (sph_gate.h): the table the kernels read with its host mirror, the gates as set, the books, the
    // per-block partial rows and the history ring (gtRingCap rows)
    DevTable<sph::GateTab> d_gtTab;
    sph::GateAcc* d_gtAcc = nullptr;
    DevBuf<unsigned long long> d_gtPart, d_gtRing;
    sph::GateTab gtTab{};                // host mirror of *d_gtTab.p (count 0: no gates, nothing is launched)
    SphGate gtSet[sph::kGateMax] = {};
    uint32_t gtRingCap = 0;

    // sph_monitor_*: the slots, and how many of them hold a monitor (0: nothing is launched, nothing enters a graph's key)
    MonitorSlot mon[sph::kMonitorMax];
    int monCount = 0;

    // sph_obstacles_*: K bodies (sph_obstacle.h ObsRec, room for kObsMax), their accumulators and the per-block partial rows of k_obstacles
    DevTable<sph::ObsRec> d_obs;
    sph::ObsAcc* d_obsAcc = nullptr;
    double* d_obsPart = nullptr;
    int obsK = 0;

    // sph_volume_* (sph_volume.h): the signed distance lattices, the device table (slots and per-body bindings) with its host mirror, and
    // the scratch of sph_mesh_distance (mesh copy and per-split partial results)
    struct VolSlot { float* d = nullptr; int dims[3] = {0, 0, 0}; float spacing[3] = {0.0f, 0.0f, 0.0f}; };
    VolSlot vols[sph::kVolMax];
    DevTable<sph::VolTable> d_volTab;
    sph::VolTable volTab{};              // host mirror of *d_volTab.p
    int volBound = 0;                    // bodies bound to a volume: k_obstacles_vol is launched instead of k_obstacles while > 0
    int obsShape[sph::kObsMax] = {0};    // shapes of the current set (a volume binds to a box only)
    // dynamic bodies (sph_obstacle.h ObsDyn): one record per body beside d_obs and the records as set (host
    // mirror); k_obstacles_finish_dyn is launched instead of k_obstacles_finish while dynCount > 0
    DevTable<sph::ObsDyn> d_dyn;
    int dynCount = 0;
    bool dynOn[sph::kObsMax] = {false};
    SphObstacleDynamics dynSet[sph::kObsMax] = {};
    // sph_volume_moments: the partial rows and the ten results
    DevBuf<double> d_momPart, d_momOut;
    int optMeshSplit = 0;                // SPH_OPT_MESH_SPLIT
    DevBuf<float> d_meshVerts, d_meshD2;
    DevBuf<uint32_t> d_meshTris;
    DevBuf<double> d_meshW;

    std::vector<SphParticle> hostInit;   // SPHFluidGPU::particles: initial state only

    // sph_state_digest (sph_state.h): two 64-bit sums per section
    DevBuf<unsigned long long> d_stateAcc;

    // timing
    struct Ev { int cls; hipEvent_t a, b; };
    std::vector<Ev> evLive;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evPool;
    double kms[SPH_K_COUNT] = {0};
    int64_t klaunch[SPH_K_COUNT] = {0};
};

namespace {

using namespace sph;

template <class T>
int DevBuf<T>::grow(SphEngine* e, size_t need) {
    if (need <= cap && p) return SPH_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    release();
    int rc;
    if ((rc = dev_alloc(&p, need))) return rc;
    cap = need;
    return SPH_OK;
}

template <class T>
int DevTable<T>::ensure(SphEngine* e, size_t count, const char* what) {
    if (p) return SPH_OK;
    int rc;
    if ((rc = dev_alloc(&p, count))) return rc;
    const hipError_t er = stage.create(e->stream, count);
    if (er == hipSuccess) return SPH_OK;
    release();
    return fail(SPH_ERR_HIP, "%s: %s", what, hipGetErrorString(er));
}
template <class T>
int DevTable<T>::send_part(SphEngine* e, size_t off, size_t bytes, size_t at) {
    const char* from = reinterpret_cast<const char*>(stage.h + (size_t)stage.cur * stage.per) + off;
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(p + at) + off, from, bytes, hipMemcpyHostToDevice, e->stream));
    return stage.commit(e->stream);
}

// The rows `span` (sph_state.h ring_span) still held by a ring of `history` rows of rowBytes each, row q in slot q mod history, to `out`,
// oldest first: at most two contiguous copies, queued on the engine's stream.  The caller synchronises.
int ring_read(SphEngine* e, const void* d_ring, size_t rowBytes, uint32_t history, RingSpan span, void* out) {
    if (!span.have) return SPH_OK;
    const uint32_t s0 = (uint32_t)(span.first % history), n0 = std::min(span.have, history - s0);
    const char* ring = static_cast<const char*>(d_ring);
    char* to = static_cast<char*>(out);
    HIP_TRY(hipMemcpyAsync(to, ring + (size_t)s0 * rowBytes, (size_t)n0 * rowBytes, hipMemcpyDeviceToHost, e->stream));
    if (span.have > n0) HIP_TRY(hipMemcpyAsync(to + (size_t)n0 * rowBytes, ring, (size_t)(span.have - n0) * rowBytes, hipMemcpyDeviceToHost, e->stream));
    return SPH_OK;
}

// What every feature that reads the sorted copy answers under the linked-list grid build; `who` is subject and verb ("gates need").
int needs_sorted_copy(const SphEngine* e, const char* who) {
    if (e->optGridBuild != 1) return SPH_OK;
    return fail(SPH_ERR_STATE, "%s the counting-sort grid build (SPH_OPT_GRID_BUILD 0): the linked-list variant keeps no sorted copy", who);
}

// Members that decide where the container walls and the grid are (for the slab exchange's reduced scan).
void container_key(const SphParams& q, float out[15]) {
    const float v[15] = {q.param_boxCenter[0], q.param_boxCenter[1], q.param_boxCenter[2], q.param_boxHalf[0], q.param_boxHalf[1], q.param_boxHalf[2],
                         q.param_boxEulerDeg[0], q.param_boxEulerDeg[1], q.param_boxEulerDeg[2], (float)q.param_shapeType,
                         q.param_shapeAux[0], q.param_shapeAux[1], q.param_shapeAux[2], q.param_h, (float)q.grid_cap};
    std::memcpy(out, v, sizeof(v));
}
// Something every rank knows to stir the fluid (an impulse, a container / grid edit, a priming exchange): whole faces for three exchanges, and one more
// event on the count every rank's plan carries (a rank that saw an event its neighbour did not is found by the plans' comparison, not by a hang).
void slab_hold(SphEngine* e) {
    e->calmHold = 3;
    e->holdEvents += 1u;
}
bool slab_ranges_usable(const SphEngine* e) {
    if (!e->slabOrderValid) return false;
    float cont[15];
    container_key(e->params, cont);
    return std::memcmp(cont, e->lastContainer, sizeof(cont)) == 0;   // same walls and same grid as the dispatch that sorted the slots
}

int flush_events(SphEngine* e) {
    if (e->evLive.empty()) return SPH_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->xstream) HIP_TRY(hipStreamSynchronize(e->xstream));
    for (auto& ev : e->evLive) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        e->kms[ev.cls] += ms;
        e->klaunch[ev.cls] += 1;
        e->evPool.emplace_back(ev.a, ev.b);
    }
    e->evLive.clear();
    return SPH_OK;
}

struct Timed {   // RAII-ish bracket around one kernel launch when SPH_OPT_TIMING is on
    SphEngine* e;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    Timed(SphEngine* e_, int cls_, hipStream_t st_ = nullptr) : e(e_), cls(cls_), st(st_ ? st_ : e_->stream) {
        if (!e->optTiming || (e->optTiming == 2 && cls != SPH_K_SPH)) return;
        if (e->evPool.empty()) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        } else {
            a = e->evPool.back().first; b = e->evPool.back().second; e->evPool.pop_back();
        }
        (void)hipEventRecord(a, st);
    }
    ~Timed() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        e->evLive.push_back({cls, a, b});
        if (e->evLive.size() >= 8192) (void)flush_events(e);
    }
};

void free_particle_buffers(SphEngine* e) {
    dev_free(e->d_aos);
    for (int b = 0; b < 2; ++b) { dev_free(e->d_pos[b]); dev_free(e->d_vel[b]); dev_free(e->d_rp[b]); dev_free(e->d_foam[b]); }
    dev_free(e->d_acc);
    dev_free(e->d_binKey); dev_free(e->d_order); dev_free(e->d_tmp);
    dev_free(e->d_slabCnt); for (auto& f : e->d_face) dev_free(f);
    e->faceCap = 0; dev_free(e->d_shapeTab); dev_free(e->d_sPV); dev_free(e->d_sOwn);
    for (auto& g : e->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
    dev_free(e->d_llNext); dev_free(e->d_llCell); dev_free(e->d_llKey);
    e->cap = 0;
}
void free_grid_buffers(SphEngine* e) {
    if (!e->graphs.empty() && e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& g : e->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);   // captured launches hold these addresses
    e->graphs.clear();
    dev_free(e->d_cellCount); dev_free(e->d_cellStart); dev_free(e->d_blockSums);
    e->allocatedCells = 0;
}

// One free function per feature (callers have drained the stream, or the function does): sph_destroy calls each.
void sample_free(SphEngine* e) { e->d_sampleIn.release(); e->d_sampleOut.release(); }
void neighbors_free(SphEngine* e) {
    e->d_slotIds.release(); e->d_nbIndices.release(); e->d_nbCnt.release(); e->d_nbOffsets.release();
    e->scanScratch.release();                                       // (the scan scratch of components and shell too: the three are freed together)
    e->nbInfo = SphNeighborInfo{};
    e->nbIndexed = false;
}
void components_free(SphEngine* e) {
    e->d_ccIds.release(); e->d_ccLabels.release(); e->d_ccRoots.release(); e->d_ccParent.release(); e->d_ccMinId.release(); e->d_ccFlag.release();
    e->d_ccWords.release(); e->d_ccStats.release(); e->d_ccOffsets.release(); e->d_ccTable.release();
    e->ccInfo = SphComponentInfo{};
    e->ccValid = false;
}
void knn_free(SphEngine* e) {
    e->d_slotIds.release(); e->d_knnIndices.release(); e->d_knnDist2.release(); e->d_knnCounts.release(); e->d_knnStats.release();
    e->knnInfo = SphKnnInfo{};
}
void shell_free(SphEngine* e) {
    e->d_shRows.release(); e->d_shIds.release(); e->d_shSlots.release(); e->d_shNrm.release(); e->d_shFlagRow.release(); e->d_shFlagSlot.release();
    e->d_shStats.release(); e->d_shOffsets.release();
    e->shellInfo = SphShellInfo{};
}
void aggregate_free(SphEngine* e) {
    e->d_aggStage.release(); e->d_aggIn.release(); e->d_aggOut.release(); e->d_aggCnt.release();
    e->d_adjKey.release(); e->d_adjCount.release(); e->d_adjSums.release(); e->d_adjStart.release(); e->d_adjTmp.release(); e->d_adjPerm.release();
    e->d_adjArg.release(); e->d_adjPts.release(); e->d_adjIn.release(); e->d_posStage.release();
}
void aniso_free(SphEngine* e) {
    e->d_anRows.release(); e->d_anSlots.release(); e->d_anStats.release();
    e->anisoInfo = SphAnisoInfo{};
}
void rays_free(SphEngine* e) {
    e->d_rayIn.release(); e->d_rayHits.release(); e->d_rayStats.release();
    e->d_rayBin.release(); e->d_rayCount.release(); e->d_rayStart.release(); e->d_rayBlockSums.release(); e->d_rayOrder.release();
    e->raysInfo = SphRaysInfo{};
    e->raysValid = false;
    e->d_spanRows.release(); e->d_spanStats.release();
    e->spansInfo = SphRaySpansInfo{};
    e->spansValid = false;
}
void surface_free(SphEngine* e) {
    e->d_surfVol.release(); e->d_surfCode.release(); e->d_surfVOff.release(); e->d_surfTile.release(); e->d_surfTileOff.release();
    e->d_surfVerts.release(); e->d_surfTris.release();
}
void stats_free(SphEngine* e) { e->d_statSums.release(); e->d_statPart.release(); e->d_statHist.release(); e->d_statCell.release(); e->d_statOut.release(); }

void tracers_free(SphEngine* e) {
    if (e->d_trRec && e->stream) (void)hipStreamSynchronize(e->stream);
    dev_free(e->d_trRec); dev_free(e->d_trPerm); dev_free(e->d_trRing); dev_free(e->d_trState); dev_free(e->d_trKey);
    e->d_trCellCount.release(); e->d_trCellStart.release(); e->d_trBlockSums.release();
    e->trM = e->trCap = e->trRingCap = 0;
    e->trK = 0; e->trS = 1; e->trSteps = e->trSorted = 0;
    e->trOrdered = false;
}

// The crest term's coefficients and books (behind a drained stream).
void diffuse_crest_free(SphEngine* e) { e->d_dfCrCoef.release(); dev_free(e->d_dfCrState); }
void diffuse_free(SphEngine* e) {
    if (e->d_dfPool && e->stream) (void)hipStreamSynchronize(e->stream);
    dev_free(e->d_dfPool); dev_free(e->d_dfScratch); dev_free(e->d_dfState); e->d_dfCoef.release();
    dev_free(e->d_dfFlag); dev_free(e->d_dfFlagStart); dev_free(e->d_dfFlagSums); dev_free(e->d_dfPart);
    e->d_dfCnt.release(); e->d_dfCntStart.release(); e->d_dfCntSums.release();
    e->dfC = 0;
    e->dfCfg = SphDiffuseConfig{};
    diffuse_crest_free(e);                                           // (the crest term goes with the pool)
    e->d_dfCrNrm.release(); e->d_dfCrFlag.release(); e->dfCrScan.release(); e->d_dfCrPart.release(); e->d_dfCrOffsets.release();
    e->d_dfCrSlots.release(); e->d_dfCrCrest.release();
    e->dfCrOn = false;
    e->dfCrCfg = SphDiffuseCrest{};
}

// The coupling's table, books and partial rows (behind a drained stream, or before anything was queued on them).
void couple_free(SphEngine* e) { e->d_cpTab.release(); dev_free(e->d_cpAcc); dev_free(e->d_cpPart); }
void scalars_free(SphEngine* e) {
    if (e->d_scVal && e->stream) (void)hipStreamSynchronize(e->stream);
    dev_free(e->d_scVal); dev_free(e->d_scSorted); e->d_scCoef.release(); dev_free(e->d_scState);
    couple_free(e);
    e->cpTab = sph::CoupleTab{};
    e->cpBuoy = false;
    e->d_scView.release(); e->d_scViewRp.release(); e->d_scSampleOut.release();
    e->scK = 0; e->scN = 0; e->scSteps = 0;
}

void gates_free(SphEngine* e) {
    if (e->d_gtTab.p && e->stream) (void)hipStreamSynchronize(e->stream);
    e->d_gtTab.release(); dev_free(e->d_gtAcc);
    e->d_gtPart.release(); e->d_gtRing.release();
    e->gtTab = sph::GateTab{};
    e->gtRingCap = 0;
}

void monitor_free(SphEngine* e, int slot) {
    MonitorSlot& s = e->mon[slot];
    if (s.d_tab.p && e->stream) (void)hipStreamSynchronize(e->stream);
    s.d_tab.release();
    s.d_points.release(); s.d_ring.release(); s.d_perm.release(); s.d_rows.release(); s.d_times.release();
    if (s.kind != SPH_MONITOR_NONE) e->monCount -= 1;
    s.kind = SPH_MONITOR_NONE; s.m = 0;
    s.dims[0] = s.dims[1] = s.dims[2] = 0;
    s.cfg = SphMonitorConfig{};
    s.tab = sph::MonitorTab{};
}
void monitors_free(SphEngine* e) {
    for (int i = 0; i < sph::kMonitorMax; ++i) monitor_free(e, i);
}

void obstacles_free(SphEngine* e) {
    if (e->d_obs.p && e->stream) (void)hipStreamSynchronize(e->stream);
    e->d_obs.release(); dev_free(e->d_obsAcc); dev_free(e->d_obsPart); e->d_dyn.release();
    e->dynCount = 0;
    for (auto& on : e->dynOn) on = false;
    e->obsK = 0;
}

// Every binding dropped (host mirror only; volumes_upload_table sends it).
void volumes_unbind_all(SphEngine* e) {
    for (int i = 0; i < sph::kVolBodies; ++i) e->volTab.bind[i] = -1;
    e->volBound = 0;
}
void volumes_free(SphEngine* e) {
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& v : e->vols) { dev_free(v.d); v = SphEngine::VolSlot{}; }
    e->d_volTab.release();
    std::memset(&e->volTab, 0, sizeof(e->volTab));
    volumes_unbind_all(e);
    e->d_meshVerts.release(); e->d_meshTris.release(); e->d_meshD2.release(); e->d_meshW.release();
    e->d_momPart.release(); e->d_momOut.release();
}

int alloc_particle_buffers(SphEngine* e, size_t n) {
    free_particle_buffers(e);
    int rc;
    if ((rc = dev_alloc(&e->d_aos, n))) return rc;
    for (int b = 0; b < 2; ++b) {
        if ((rc = dev_alloc(&e->d_pos[b], n))) return rc;
        if ((rc = dev_alloc(&e->d_vel[b], n))) return rc;
        if ((rc = dev_alloc(&e->d_rp[b], n))) return rc;
        if ((rc = dev_alloc(&e->d_foam[b], n))) return rc;
    }
    if ((rc = dev_alloc(&e->d_acc, n))) return rc;
    if ((rc = dev_alloc(&e->d_binKey, n))) return rc;
    if ((rc = dev_alloc(&e->d_order, n))) return rc;
    if ((rc = dev_alloc(&e->d_tmp, n))) return rc;
    if ((rc = dev_alloc(&e->d_slabCnt, kSlabCounters))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_slabCnt, 0, kSlabCounters * sizeof(uint32_t), e->stream));
    e->cap = n;
    return SPH_OK;
}

// cellHead realloc of SPHFluid3D.cpp:440-447 (only when the cell count changed)
int local_cells(const SphEngine* e) {
    return e->slab ? e->grid.dims[0] * e->grid.dims[1] * (e->z1 - e->z0 + 2) : e->grid.numCells;
}

int ensure_grid_buffers(SphEngine* e) {
    const int want = local_cells(e);
    if (want == e->allocatedCells && e->d_cellCount) return SPH_OK;
    free_grid_buffers(e);
    const size_t C = (size_t)want;
    int rc;
    if ((rc = dev_alloc(&e->d_cellCount, C))) return rc;
    if ((rc = dev_alloc(&e->d_cellStart, C + 1))) return rc;
    if ((rc = dev_alloc(&e->d_blockSums, (size_t)blocks_for(C, kScanTile) + 1))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_cellCount, 0, C * sizeof(uint32_t), e->stream));
    e->allocatedCells = want;
    return SPH_OK;
}

constexpr long long kMaxCells = 1ll << 30;       // int32 cell indices and 4-byte-per-cell buffers stay far from overflow
constexpr size_t kMaxParticles = (size_t)1 << 30;
int validate_params(const SphParams& p) {
    if (!(p.param_h > 0.0f)) return fail(SPH_ERR_ARG, "param_h must be > 0");
    SphGridInfo g;
    compute_grid_extents(p, g);
    for (int a = 0; a < 3; ++a)
        if (g.dims[a] > 1024) return fail(SPH_ERR_CAPACITY, "grid axis %d has %d cells; the engine packs cell coordinates in 10 bits per axis (max 1024)", a, g.dims[a]);
    const long long nc = (long long)g.dims[0] * g.dims[1] * g.dims[2];
    if (nc > kMaxCells) return fail(SPH_ERR_CAPACITY, "grid of %d x %d x %d cells exceeds %lld cells (grid_cap %d)", g.dims[0], g.dims[1], g.dims[2], kMaxCells, p.grid_cap);
    return SPH_OK;
}

int set_particles(SphEngine* e, const SphParticle* host, size_t n) {
    int rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (n > e->cap || !e->d_aos) { if ((rc = alloc_particle_buffers(e, n))) return rc; }
    e->n = n;
    e->hostInit.assign(host, host + n);
    if (n) HIP_TRY(hipMemcpyAsync(e->d_aos, host, n * sizeof(SphParticle), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // `host` may be a temporary of the caller
    e->aosValid = true; e->internalValid = false; e->accValid = false; e->cur = 0;
    return SPH_OK;
}

int import_state(SphEngine* e) {
    if (e->internalValid) return SPH_OK;
    if (e->slab) return fail(SPH_ERR_STATE, "slab engine without a valid state");
    if (!e->aosValid) return fail(SPH_ERR_STATE, "neither the AoS nor the internal state is valid");
    if (e->n) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_import, dim3(blocks_for(e->n)), dim3(kBlock), 0, e->stream, e->d_aos, e->d_pos[e->cur],
                           e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur], e->idBase, (int)e->n);
    }
    HIP_TRY(hipGetLastError());
    e->internalValid = true;
    e->accValid = false;
    return SPH_OK;
}

// The counting sort's exclusive scan of `count` (C cells) into start[0..C]; k_scan_apply leaves count zero again.
void launch_cell_scan(SphEngine* e, uint32_t* count, uint32_t* blockSums, uint32_t* start, int C, uint32_t total) {
    const int sb = blocks_for((size_t)C, kScanTile);
    const int rawSums = sb <= kScanFusedBlocks ? 1 : 0;
    hipLaunchKernelGGL(k_scan_reduce, dim3(sb), dim3(kBlock), 0, e->stream, count, blockSums, C);
    if (!rawSums) hipLaunchKernelGGL(k_scan_blocksums, dim3(1), dim3(kBlock), 0, e->stream, blockSums, sb);
    hipLaunchKernelGGL(k_scan_apply, dim3(sb), dim3(kBlock), 0, e->stream, count, blockSums, start, C, total, rawSums);
}

// ClearGrid + BuildGrid as a counting sort: after this, d_cellStart/d_order describe the
// current state buffer.
// commitLive (z-slab dispatch only): k_rank also stores the live count as the new slots-in-use count of the exchange.
// orderAll (sph_statistics only): k_rank writes order[] for every slot, not only for ghosts (the exact density is gathered through it).
int build_grid(SphEngine* e, const SimK& k, bool commitLive = false, bool orderAll = false) {
    const int n = (int)(e->slab ? e->nSlots : e->n), C = k.numCells;
    const int nb = blocks_for(n);
    const bool sortedCopy = e->optGridBuild == 0;     // k_rank also writes the sorted copy the SPH pass reads
    if (sortedCopy && (e->sortedCap < e->cap || !e->d_sPV)) {
        int rc;
        dev_free(e->d_sPV); dev_free(e->d_sOwn);
        e->d_sPV = e->d_sOwn = nullptr; e->sortedCap = 0;
        if ((rc = dev_alloc(&e->d_sPV, 2 * e->cap)) || (rc = dev_alloc(&e->d_sOwn, e->cap))) return rc;
        e->sortedCap = e->cap;
    }
    if (n) {
        Timed t(e, SPH_K_BIN);
        hipLaunchKernelGGL(k_bin, dim3(nb), dim3(kBlock), 0, e->stream, k, e->d_pos[e->cur], e->d_binKey, e->d_cellCount, n,
                           e->slab ? e->d_slabCnt + kSlabCntLive : (const uint32_t*)nullptr);
    }
    {
        Timed t(e, SPH_K_SCAN);
        launch_cell_scan(e, e->d_cellCount, e->d_blockSums, e->d_cellStart, C, (uint32_t)n);
    }
    if (n) {
        Timed t(e, SPH_K_SCATTER);
        hipLaunchKernelGGL(k_scatter, dim3(nb), dim3(kBlock), 0, e->stream, e->d_binKey, e->d_cellStart, e->d_tmp, n,
                           e->slab ? e->d_slabCnt + kSlabCntLive : (const uint32_t*)nullptr);
        if (sortedCopy && orderAll) {
            hipLaunchKernelGGL((k_rank<true, true>), dim3(nb), dim3(kBlock), 0, e->stream, e->d_tmp, e->d_cellStart, e->d_order, n, C,
                               e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur], e->d_sPV, e->d_sOwn, k.gx, k.gy,
                               (uint32_t*)nullptr);
        } else if (sortedCopy) {
            hipLaunchKernelGGL((k_rank<true>), dim3(nb), dim3(kBlock), 0, e->stream, e->d_tmp, e->d_cellStart, e->d_order, n, C,
                               e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur], e->d_sPV, e->d_sOwn, k.gx, k.gy,
                               (commitLive && e->slab) ? e->d_slabCnt + kSlabCntLive : (uint32_t*)nullptr);
        } else {
            hipLaunchKernelGGL((k_rank<false>), dim3(nb), dim3(kBlock), 0, e->stream, e->d_tmp, e->d_cellStart, e->d_order, n, C,
                               nullptr, e->d_vel[e->cur], nullptr, nullptr, nullptr, nullptr, k.gx, k.gy,
                               (commitLive && e->slab) ? e->d_slabCnt + kSlabCntLive : (uint32_t*)nullptr);
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- tracers (sph_tracer.h) --------------------------------------------------------------------
// The processing order: tracers sorted by the cell they are in, re-sorted when kTracerRefresh substeps have passed since the last sort.
// Never launched while sph_dispatch_n captures (a graph would replay the sort at every call): sph_dispatch_n sorts before it replays.
int tracers_order(SphEngine* e, const SimK& k) {
    if (!e->trM || e->capturing) return SPH_OK;
    if (e->trOrdered && e->trSteps - e->trSorted < (uint64_t)kTracerRefresh) return SPH_OK;
    const int C = k.numCells;
    int rc;
    if (e->d_trCellStart.cap < (size_t)C + 1) {              // (grown last: a failed growth is tried again)
        if ((rc = e->d_trCellCount.grow(e, (size_t)C)) || (rc = e->d_trBlockSums.grow(e, (size_t)blocks_for((size_t)C, kScanTile) + 1)) ||
            (rc = e->d_trCellStart.grow(e, (size_t)C + 1))) return rc;
        HIP_TRY(hipMemsetAsync(e->d_trCellCount.p, 0, (size_t)C * sizeof(uint32_t), e->stream));    // (k_scan_apply leaves it zero again)
    }
    const uint32_t m = (uint32_t)e->trM;
    Timed t(e, SPH_K_OTHER);
    hipLaunchKernelGGL(k_tracer_bin, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_trRec, e->d_trKey, e->d_trCellCount.p, m);
    launch_cell_scan(e, e->d_trCellCount.p, e->d_trBlockSums.p, e->d_trCellStart.p, C, m);
    hipLaunchKernelGGL(k_tracer_scatter, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, (const uint2*)e->d_trKey, e->d_trCellStart.p, e->d_trPerm, m);
    HIP_TRY(hipGetLastError());
    e->trSorted = e->trSteps;
    e->trOrdered = true;
    return SPH_OK;
}

// One substep's tracer work, behind build_grid of that substep: advect on the sorted copy of the entry state, then advance the device counter.
int tracers_advect(SphEngine* e, const SimK& k, float dt) {
    int rc;
    if ((rc = tracers_order(e, k))) return rc;
    const uint32_t m = (uint32_t)e->trM;
    {
        Timed t(e, SPH_K_OTHER);
        if (e->trIntegrator == SPH_TRACER_MIDPOINT)
            hipLaunchKernelGGL((k_tracer_advect<true>), dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, e->d_cellStart, dt,
                               (const uint32_t*)e->d_trPerm, e->d_trRec, e->d_trRing, (const uint32_t*)e->d_trState, m);
        else
            hipLaunchKernelGGL((k_tracer_advect<false>), dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, e->d_cellStart, dt,
                               (const uint32_t*)e->d_trPerm, e->d_trRec, e->d_trRing, (const uint32_t*)e->d_trState, m);
        hipLaunchKernelGGL(k_tracer_tick, dim3(1), dim3(64), 0, e->stream, e->d_trState, e->trK, e->trS);
    }
    HIP_TRY(hipGetLastError());
    e->trSteps += 1;
    return SPH_OK;
}

// ---- what the shell pass inside the substep shares with the queries (sph_query.h, sph_shell.h) ----
NbK make_nbk(const SphEngine* e, float radius, int stencil, int flags, size_t n) { return NbK{radius * radius, stencil, flags, e->idBase, (uint32_t)n}; }
// The three launches of the 64-bit exclusive scan of cnt[0 .. rows) into offsets[0 .. rows], rows > 0, on scratch grown for `rows`
// (no bracket, no synchronisation); returns where the totals lie on the device.
unsigned long long* scan_counts64_launch(SphEngine* e, const ScanScratch& scratch, const uint32_t* cnt, size_t rows, long long* offsets) {
    const int tiles = blocks_for(rows, kScanTile);
    unsigned long long *tileSums = scratch.tileSums.p, *totals = tileSums + tiles;
    uint32_t* tileMax = scratch.tileMax.p;
    hipLaunchKernelGGL(k_neighbors_scan_reduce, dim3(tiles), dim3(kBlock), 0, e->stream, cnt, rows, tileSums, tileMax);
    hipLaunchKernelGGL(k_neighbors_scan_tiles, dim3(1), dim3(kBlock), 0, e->stream, tileSums, (const uint32_t*)tileMax, tiles, totals);
    hipLaunchKernelGGL(k_neighbors_scan_apply, dim3(tiles), dim3(kBlock), 0, e->stream, cnt, rows, (const unsigned long long*)tileSums,
                       (const unsigned long long*)totals, offsets);
    return totals;
}
// The radius in force of a shell config (radius <= 0: h) and the constants of its kernels.
float shell_radius(const SphShellConfig& cfg, float h) { return cfg.radius <= 0.0f ? h : cfg.radius; }
ShellK shell_consts(const SphShellConfig& cfg, float radius) { return ShellK{radius, radius * radius, cfg.offset, cfg.minCount}; }

// ---- spray, foam and bubbles (sph_diffuse.h) -----------------------------------------------------
// The crest term's shell pass as a shell config.
SphShellConfig diffuse_crest_shell_config(const SphDiffuseCrest& c) { return SphShellConfig{c.radius, c.offset, c.minCount, c.flags}; }
// The launch arguments of the crest term's shell pass at the current params; false: no radius of this grid.
bool diffuse_crest_args(const SphEngine* e, float cellSize, float* radius, int* stencil) {
    *radius = shell_radius(diffuse_crest_shell_config(e->dfCrCfg), e->params.param_h);
    *stencil = sph::neighbor_stencil(*radius, cellSize);
    return *stencil != 0;
}

// The scratch of the crest term's shell pass for n slots, grown in the eager run in front of the substep's timed bracket.
int diffuse_crest_scratch(SphEngine* e, uint32_t n) {
    int rc;
    if (e->d_dfCrOffsets.cap < (size_t)n + 1) {              // (grown last: a failed growth is tried again; never while capturing)
        if (e->capturing) return fail(SPH_ERR_STATE, "diffuse crest scratch missing during a graph capture");
        if ((rc = e->d_dfCrNrm.grow(e, n)) || (rc = e->d_dfCrFlag.grow(e, n)) || (rc = e->d_dfCrSlots.grow(e, n)) || (rc = e->d_dfCrCrest.grow(e, n)) ||
            (rc = e->dfCrScan.grow(e, n)) || (rc = e->d_dfCrPart.grow(e, (size_t)blocks_for(n))) ||
            (rc = e->d_dfCrOffsets.grow(e, (size_t)n + 1))) return rc;
        // (a first substep that does not act leaves the passes idle: the scan and the count must still read defined words)
        HIP_TRY(hipMemsetAsync(e->d_dfCrNrm.p, 0, e->d_dfCrNrm.cap * sizeof(float4), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_dfCrFlag.p, 0, e->d_dfCrFlag.cap * sizeof(uint32_t), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_dfCrSlots.p, 0, e->d_dfCrSlots.cap * sizeof(int32_t), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_dfCrCrest.p, 0, e->d_dfCrCrest.cap * sizeof(float), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_dfCrOffsets.p, 0, e->d_dfCrOffsets.cap * sizeof(long long), e->stream));
    }
    return SPH_OK;
}
// The crest term's launches in front of the count: pass 1 by slot, the scan of the shell flags (its total stays behind the offsets),
// the compaction of the shell slots, pass 2 over them.  All sized by n; on a substep that does not act the two passes return at once.
// sph_shell.h and sph_diffuse.h meet here, through plain arrays.
int diffuse_crest_shell(SphEngine* e, const SimK& k, uint32_t n) {
    float radius = 0.0f;
    int stencil = 0;
    if (!diffuse_crest_args(e, k.cellSize, &radius, &stencil))
        return fail(SPH_ERR_STATE, "diffuse crest radius %g is above three cells (%g) of this grid", (double)radius, (double)(3.0f * k.cellSize));
    if (!n) return SPH_OK;
    const SphShellConfig cfg = diffuse_crest_shell_config(e->dfCrCfg);
    const NbK nb = make_nbk(e, radius, stencil, cfg.flags, n);
    const ShellK sk = shell_consts(cfg, radius);
    const dim3 grid(blocks_for(n)), block(kBlock);
    const float4* pv = (const float4*)e->d_sPV;
    const uint32_t* cellStart = (const uint32_t*)e->d_cellStart;
    const uint32_t* counter = (const uint32_t*)e->d_dfState + DF_STEP_LO;
    const uint32_t* period = &e->d_dfCrCoef.p->every;         // (an address, not a load: device memory)
    hipLaunchKernelGGL(k_shell_slot_gather, grid, block, 0, e->stream, k, nb, sk, pv, cellStart, (const float4*)e->d_sOwn, counter, period, e->d_dfCrNrm.p,
                       e->d_dfCrFlag.p);
    (void)scan_counts64_launch(e, e->dfCrScan, (const uint32_t*)e->d_dfCrFlag.p, (size_t)n, e->d_dfCrOffsets.p);
    hipLaunchKernelGGL(k_shell_compact, grid, block, 0, e->stream, (const uint32_t*)e->d_dfCrFlag.p, (const long long*)e->d_dfCrOffsets.p, (size_t)n, e->d_dfCrSlots.p);
    hipLaunchKernelGGL(k_shell_slot_crest, grid, block, 0, e->stream, k, nb, sk, pv, cellStart, (const float4*)e->d_dfCrNrm.p, (const int32_t*)e->d_dfCrSlots.p,
                       (const long long*)e->d_dfCrOffsets.p + n, counter, period, e->d_dfCrCrest.p);
    return SPH_OK;
}

// One substep's work on the pool, behind build_grid of that substep: advance into the scratch pool, count the children (with the crest
// term on: behind its shell pass), scan both, compact the survivors back, emit the newborn behind them, tick.  Sized by C and N alone.
int diffuse_step(SphEngine* e, const SimK& k, float dt, uint32_t n) {
    const uint32_t C = e->dfC;
    int rc;
    if (e->d_dfCntStart.cap < (size_t)n + 1) {               // (grown last: a failed growth is tried again; never while capturing: the eager run before has grown them)
        if (e->capturing) return fail(SPH_ERR_STATE, "diffuse scratch missing during a graph capture");
        if ((rc = e->d_dfCnt.grow(e, (size_t)n + 8)) || (rc = e->d_dfCntSums.grow(e, (size_t)blocks_for((size_t)n, kScanTile) + 1)) ||
            (rc = e->d_dfCntStart.grow(e, (size_t)n + 1))) return rc;
        HIP_TRY(hipMemsetAsync(e->d_dfCnt.p, 0, e->d_dfCnt.cap * sizeof(uint32_t), e->stream));     // (k_scan_apply leaves it zero again)
    }
    const bool crest = e->dfCrOn;
    if (crest && (rc = diffuse_crest_scratch(e, n))) return rc;
    // one bracket per substep: around everything, or (SPH_OPT_DIFFUSE_TIMED, measurements) around the advance or around the rest
    std::unique_ptr<Timed> t;
    if (e->optDiffuseTimed != 2) t.reset(new Timed(e, SPH_K_OTHER));
    const int cb = blocks_for(C), nb = blocks_for(n);
    hipLaunchKernelGGL(k_diffuse_advance, dim3(cb), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, dt,
                       (const DiffuseCoef*)e->d_dfCoef.p, (const uint32_t*)e->d_dfState, (const float4*)e->d_dfPool, e->d_dfScratch, e->d_dfFlag, e->d_dfPart, C);
    if (e->optDiffuseTimed == 1) t.reset();
    if (e->optDiffuseTimed == 2) t.reset(new Timed(e, SPH_K_OTHER));
    if (crest && (rc = diffuse_crest_shell(e, k, n))) return rc;
    if (n && crest)
        hipLaunchKernelGGL(k_diffuse_count_crest, dim3(nb), dim3(kBlock), 0, e->stream, (const float4*)e->d_sPV, (const float4*)e->d_sOwn, dt,
                           (const DiffuseCoef*)e->d_dfCoef.p, (const DiffuseCrestCoef*)e->d_dfCrCoef.p, (const uint32_t*)e->d_dfState,
                           (const float4*)e->d_dfCrNrm.p, (const float*)e->d_dfCrCrest.p, e->d_dfCnt.p, e->d_dfCrPart.p, e->idBase, n);
    else if (n)
        hipLaunchKernelGGL(k_diffuse_count, dim3(nb), dim3(kBlock), 0, e->stream, (const float4*)e->d_sPV, (const float4*)e->d_sOwn, dt,
                           (const DiffuseCoef*)e->d_dfCoef.p, (const uint32_t*)e->d_dfState, e->d_dfCnt.p, e->idBase, n);
    launch_cell_scan(e, e->d_dfFlag, e->d_dfFlagSums, e->d_dfFlagStart, (int)C, C);
    if (n) launch_cell_scan(e, e->d_dfCnt.p, e->d_dfCntSums.p, e->d_dfCntStart.p, (int)n, n);
    else HIP_TRY(hipMemsetAsync(e->d_dfCntStart.p, 0, sizeof(uint32_t), e->stream));
    hipLaunchKernelGGL(k_diffuse_compact, dim3(cb), dim3(kBlock), 0, e->stream, (const float4*)e->d_dfScratch, (const uint32_t*)e->d_dfFlagStart,
                       (const uint32_t*)e->d_dfState, e->d_dfPool, C);
    if (n)
        hipLaunchKernelGGL(k_diffuse_emit, dim3(nb), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, (const float4*)e->d_sOwn,
                           (const DiffuseCoef*)e->d_dfCoef.p, (const uint32_t*)e->d_dfState, (const uint32_t*)e->d_dfCntStart.p,
                           (const uint32_t*)e->d_dfFlagStart, e->d_dfPool, e->idBase, n, C);
    if (crest)                                                          // (in front of the tick: it reads the counter the tick advances)
        hipLaunchKernelGGL(k_diffuse_crest_tick, dim3(1), dim3(kBlock), 0, e->stream, (const uint32_t*)e->d_dfState, (const DiffuseCrestCoef*)e->d_dfCrCoef.p,
                           (const uint32_t*)e->d_dfCrPart.p, (uint32_t)(n ? nb : 0), (const long long*)e->d_dfCrOffsets.p + n, n, e->d_dfCrState);
    hipLaunchKernelGGL(k_diffuse_tick, dim3(1), dim3(kBlock), 0, e->stream, e->d_dfState, (const uint32_t*)e->d_dfPart, (uint32_t)cb,
                       (const uint32_t*)e->d_dfFlagStart, (const uint32_t*)e->d_dfCntStart.p, n, C);
    t.reset();
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- diffusing scalars (sph_scalar.h) -------------------------------------------------------------
// One substep's scalar work, behind build_grid of that substep: gather the values into slot order, then the neighbour sweep on the sorted copy.
template <int K>
void scalars_launch(SphEngine* e, const SimK& k, float dt, uint32_t n) {
    hipLaunchKernelGGL((k_scalar_gather<K>), dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, (const float4*)e->d_sOwn, (const float*)e->d_scVal, e->d_scSorted,
                       e->d_scState, e->idBase, n);
    const float kLap = scalar_klap(e->params.param_mass, e->params.param_h);
    if (e->optScalarSweep == 1)
        hipLaunchKernelGGL((k_scalar_sweep_staged<K>), dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, (const float4*)e->d_sOwn,
                           (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, (const ScalarCoef*)e->d_scCoef.p, kLap, dt, e->d_scVal, e->d_scState,
                           e->idBase, n);
    else
        hipLaunchKernelGGL((k_scalar_sweep<K>), dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, (const float4*)e->d_sOwn,
                           (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, (const ScalarCoef*)e->d_scCoef.p, kLap, dt, e->d_scVal, e->d_scState,
                           e->idBase, n);
}
// The gather alone, outside a substep (sampling, on the grid of the current state): the diffusion number is left alone.
template <int K>
void scalars_gather_launch(SphEngine* e, uint32_t n) {
    hipLaunchKernelGGL((k_scalar_gather<K>), dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, (const float4*)e->d_sOwn, (const float*)e->d_scVal, e->d_scSorted,
                       (uint32_t*)nullptr, e->idBase, n);
}
void scalars_gather_now(SphEngine* e, uint32_t n) {
    switch (e->scK) {
    case 1: scalars_gather_launch<1>(e, n); break;
    case 2: scalars_gather_launch<2>(e, n); break;
    case 3: scalars_gather_launch<3>(e, n); break;
    default: scalars_gather_launch<4>(e, n); break;
    }
}
int scalars_step(SphEngine* e, const SimK& k, float dt) {
    const uint32_t n = (uint32_t)e->n;
    if (n) {
        Timed t(e, SPH_K_OTHER);
        switch (e->scK) {
        case 1: scalars_launch<1>(e, k, dt, n); break;
        case 2: scalars_launch<2>(e, k, dt, n); break;
        case 3: scalars_launch<3>(e, k, dt, n); break;
        default: scalars_launch<4>(e, k, dt, n); break;
        }
    }
    HIP_TRY(hipGetLastError());
    e->scSteps += 1;
    return SPH_OK;
}

// The substep's scalar work on the CPU: the grid as the counting sort leaves it (cells ascending, members ascending by index), the
// gathered copy, then scalar_pair / scalar_finish per target in slot order.
template <int K>
float scalars_step_loop(const SimK& k, float kLap, float dt, const sph::ScalarCoef& co, const SphParticle* P, size_t n, float* values) {
    const sph::HostGrid grid(k, P, n);
    const std::vector<uint32_t>& order = grid.order;
    std::vector<float> pv(4 * n), sC((size_t)(K + 1) * n);
    for (size_t q = 0; q < n; ++q) {
        const SphParticle& p = P[order[q]];
        pv[4 * q] = p.pos[0]; pv[4 * q + 1] = p.pos[1]; pv[4 * q + 2] = p.pos[2];
        pv[4 * q + 3] = p.density > 0.0f ? 1.0f / p.density : 0.0f;
        for (int c = 0; c < K; ++c) sC[q * (K + 1) + c] = values[(size_t)order[q] * K + c];
        sC[q * (K + 1) + K] = p.isGhost != 0 ? 0.0f : 1.0f;
    }
    uint32_t best = 0u;
    for (size_t q = 0; q < n; ++q) {
        const float* X = &pv[4 * q];
        const float* ci = &sC[q * (K + 1)];
        if (!(ci[K] > 0.0f) || !sph::float_finite(X[0]) || !sph::float_finite(X[1]) || !sph::float_finite(X[2]) || !(X[3] > 0.0f)) continue;
        float a[K], W = 0.0f;
        for (int c = 0; c < K; ++c) a[c] = 0.0f;
        grid.rows(1, X, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                if (j == q) continue;
                const float* Y = &pv[4 * (size_t)j];
                const float* cj = &sC[(size_t)j * (K + 1)];
                sph::scalar_pair<K>(k.h, k.h2, X[0], X[1], X[2], X[3], ci, Y[0], Y[1], Y[2], cj[K] > 0.0f ? Y[3] : 0.0f, cj, a, W);
            }
        });
        float out[K];
        const float s = sph::scalar_finish<K>(co, kLap, dt, ci, a, W, out);
        for (int c = 0; c < K; ++c) values[(size_t)order[q] * K + c] = out[c];
        uint32_t bits;
        std::memcpy(&bits, &s, 4);
        best = std::max(best, bits);
    }
    float mx;
    std::memcpy(&mx, &best, 4);
    return mx;
}

// The coupling step on host records (arguments already checked): sources in order, then the kick, record by record in index order.
template <int K>
void couple_host_loop(const sph::CoupleTab& tab, bool buoy, const sph::ObsRec* recs, float dt, float gx, float gy, float gz, SphParticle* P, size_t n,
                             float* values, double* sums, uint64_t* hits) {
    for (size_t i = 0; i < n; ++i) {
        SphParticle& p = P[i];
        if (p.isGhost != 0 || !std::isfinite(p.pos[0]) || !std::isfinite(p.pos[1]) || !std::isfinite(p.pos[2])) continue;
        float cv[K];
        for (int k = 0; k < K; ++k) cv[k] = values[i * K + k];
        for (int s = 0; s < tab.nSrc; ++s) {
            const sph::CoupleSrc& S = tab.src[s];
            if (!sph::couple_inside(S, S.body >= 0 ? recs + S.body : nullptr, p.pos[0], p.pos[1], p.pos[2])) continue;
            const float old = cv[S.channel];
            if (!std::isfinite(old)) continue;
            const float now = sph::couple_apply(S, dt, old);
            cv[S.channel] = now;
            values[i * K + S.channel] = now;
            sums[s] += (double)now - (double)old;
            hits[s] += 1u;
        }
        if (buoy) {
            float vx = p.vel[0], vy = p.vel[1], vz = p.vel[2];
            if (sph::couple_kick<K>(tab.beta, tab.ref, cv, dt, gx, gy, gz, vx, vy, vz)) { p.vel[0] = vx; p.vel[1] = vy; p.vel[2] = vz; }
        }
    }
}

// ---- obstacles (sph_obstacle.h) -------------------------------------------------------------------
// What obs_body_step needs of the parameters: gravity, the container's oriented box as the grid sees it, the wall restitution.
void obstacle_world(const SphParams& p, sph::ObsWorld& W) {
    W.g[0] = p.param_gravityX; W.g[1] = p.param_gravityY; W.g[2] = p.param_gravityZ;
    for (int a = 0; a < 3; ++a) W.bc[a] = p.param_boxCenter[a];
    sph::rotation_mat3(p.param_boxEulerDeg, W.A);
    sph::effective_half(p, W.half);
    W.rest = p.param_wallRestitution;
}
// One substep's obstacle step on the pass's output state: k_obstacles, then the one-block finish (sums, accumulators, pose advance).
int obstacles_step(SphEngine* e, float4* pos, float4* vel, int n, float dt) {
    const int rows = n > 0 ? std::min(kObsGrid, blocks_for((size_t)n, kObsSweep)) : 0;
    {
        Timed t(e, SPH_K_OTHER);
        if (rows && e->volBound > 0)
            hipLaunchKernelGGL(k_obstacles_vol, dim3(rows), dim3(kObsBlock), 0, e->stream, (const ObsRec*)e->d_obs.p, (const VolTable*)e->d_volTab.p, e->obsK,
                               e->params.param_mass, pos, vel, n, e->d_obsPart);
        else if (rows) hipLaunchKernelGGL(k_obstacles, dim3(rows), dim3(kObsBlock), 0, e->stream, (const ObsRec*)e->d_obs.p, e->obsK, e->params.param_mass, pos, vel, n,
                                     e->d_obsPart);
        if (e->dynCount > 0) {                                       // (the finish that also steps the dynamic bodies)
            ObsWorld W;
            obstacle_world(e->params, W);
            hipLaunchKernelGGL(k_obstacles_finish_dyn, dim3(1), dim3(kObsFinishBlock), 0, e->stream, e->d_obs.p, (const ObsDyn*)e->d_dyn.p, W, e->obsK, dt,
                               (const double*)e->d_obsPart, rows, e->d_obsAcc);
        } else
        hipLaunchKernelGGL(k_obstacles_finish, dim3(1), dim3(kObsFinishBlock), 0, e->stream, e->d_obs.p, e->obsK, dt, (const double*)e->d_obsPart, rows, e->d_obsAcc);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- active scalars (sph_couple.h) -------------------------------------------------------------------
// A source bound to a body the obstacle set does not have: the dispatch is refused before anything is enqueued.
int couple_refused(const SphEngine* e) {
    for (int i = 0; i < e->cpTab.nSrc; ++i)
        if (e->cpTab.src[i].body >= e->obsK)
            return fail(SPH_ERR_STATE, "scalar source %d rides on obstacle %d, the set has %d", i, e->cpTab.src[i].body, e->obsK);
    return SPH_OK;
}
template <int K>
void couple_launch(SphEngine* e, int rows, bool src, float4* pos, float4* vel, int n, float dt) {
    const SphParams& p = e->params;
    const dim3 grid(rows), block(kObsBlock);
    const CoupleTab* tab = e->d_cpTab.p;
    const ObsRec* bodies = e->d_obs.p;
    if (src && e->cpBuoy)
        hipLaunchKernelGGL((k_scalar_couple<K, true, true>), grid, block, 0, e->stream, tab, bodies, e->obsK, dt, p.param_gravityX, p.param_gravityY, p.param_gravityZ,
                           (const float4*)pos, vel, e->d_scVal, e->idBase, n, e->d_cpPart);
    else if (src)
        hipLaunchKernelGGL((k_scalar_couple<K, true, false>), grid, block, 0, e->stream, tab, bodies, e->obsK, dt, p.param_gravityX, p.param_gravityY, p.param_gravityZ,
                           (const float4*)pos, vel, e->d_scVal, e->idBase, n, e->d_cpPart);
    else
        hipLaunchKernelGGL((k_scalar_couple<K, false, true>), grid, block, 0, e->stream, tab, bodies, e->obsK, dt, p.param_gravityX, p.param_gravityY, p.param_gravityZ,
                           (const float4*)pos, vel, e->d_scVal, e->idBase, n, e->d_cpPart);
}
// One substep's coupling step on the pass's output state: k_scalar_couple, then (with sources) the one-block finish of the books.
int couple_step(SphEngine* e, float4* pos, float4* vel, int n, float dt) {
    const bool src = e->cpTab.nSrc > 0;
    const int rows = n > 0 ? std::min(kObsGrid, blocks_for((size_t)n, kObsSweep)) : 0;
    {
        Timed t(e, SPH_K_OTHER);
        if (rows) {
            switch (e->scK) {
            case 1: couple_launch<1>(e, rows, src, pos, vel, n, dt); break;
            case 2: couple_launch<2>(e, rows, src, pos, vel, n, dt); break;
            case 3: couple_launch<3>(e, rows, src, pos, vel, n, dt); break;
            default: couple_launch<4>(e, rows, src, pos, vel, n, dt); break;
            }
        }
        if (src) hipLaunchKernelGGL(k_scalar_couple_finish, dim3(1), dim3(kCoupleFinishBlock), 0, e->stream, dt, (const double*)e->d_cpPart, rows, e->d_cpAcc);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- flow gates (sph_gate.h) -------------------------------------------------------------------------
template <int K>
void gates_launch(SphEngine* e, int rows, const float4* pos, const float4* vel, int n) {
    hipLaunchKernelGGL((k_gates<K>), dim3(rows), dim3(kGateBlock), 0, e->stream, (const GateTab*)e->d_gtTab.p, pos, vel, (const float4*)e->d_sPV,
                       (const float*)e->d_scVal, e->idBase, n, e->d_gtPart.p);
}
// One substep's gate step on the pass's output state and the sorted copy of its entry state: k_gates, then the one-block finish of the
// books and of the ring.  It writes no particle state.
int gates_step(SphEngine* e, const float4* pos, const float4* vel, int n, float dt) {
    const int rows = n > 0 ? std::min(kGateGrid, blocks_for((size_t)n, kGateSweep)) : 0;
    {
        Timed t(e, SPH_K_OTHER);
        if (rows) {
            switch (e->scK) {
            case 0: gates_launch<0>(e, rows, pos, vel, n); break;
            case 1: gates_launch<1>(e, rows, pos, vel, n); break;
            case 2: gates_launch<2>(e, rows, pos, vel, n); break;
            case 3: gates_launch<3>(e, rows, pos, vel, n); break;
            default: gates_launch<4>(e, rows, pos, vel, n); break;
            }
        }
        hipLaunchKernelGGL(k_gates_finish, dim3(1), dim3(kGateFinishBlock), 0, e->stream, dt, (const unsigned long long*)e->d_gtPart.p, rows,
                           (const GateTab*)e->d_gtTab.p, e->d_gtAcc, e->d_gtRing.p, e->gtRingCap);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- field monitors (sph_monitor.h) ---------------------------------------------------------------------
// One substep's monitor work, behind build_grid of that substep: per slot the sampling launch (it returns at once in a non-acting
// substep: the decision is in device memory) and the one-thread tick.  It writes no particle state.
int monitors_step(SphEngine* e, const SimK& k, float dt) {
    for (int i = 0; i < kMonitorMax; ++i) {
        MonitorSlot& s = e->mon[i];
        if (s.kind == SPH_MONITOR_NONE) continue;
        Timed t(e, SPH_K_OTHER);
        if (s.kind == SPH_MONITOR_POINTS)
            hipLaunchKernelGGL(k_monitor_points, dim3(blocks_for(s.m)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                               (const MonitorTab*)s.d_tab.p, (const float4*)s.d_points.p, (const uint32_t*)s.d_perm.p, s.d_rows.p, s.d_ring.p, (uint32_t)s.m);
        else
            hipLaunchKernelGGL(k_monitor_lattice, dim3((unsigned)std::min<long long>(s.tab.L.nBricks, 1ll << 20)), dim3(kBlock), 0, e->stream, k,
                               (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const MonitorTab*)s.d_tab.p, s.d_rows.p, s.d_ring.p);
        hipLaunchKernelGGL(k_monitor_tick, dim3(1), dim3(64), 0, e->stream, s.d_tab.p, s.d_times.p, dt);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int writeback(SphEngine* e) {
    if (e->slab) return fail(SPH_ERR_STATE, "a slab engine has no local 80-byte array: use sph_slab_download");
    if (e->aosValid) return SPH_OK;
    if (!e->internalValid) return fail(SPH_ERR_STATE, "no valid particle state");
    if (!e->accValid) return fail(SPH_ERR_STATE, "internal acc buffer is stale");
    if (e->n) {
        Timed t(e, SPH_K_WRITEBACK);
        hipLaunchKernelGGL(k_writeback, dim3(blocks_for(e->n)), dim3(kBlock), 0, e->stream, e->d_aos, e->d_pos[e->cur], e->d_vel[e->cur],
                           e->d_rp[e->cur], e->d_foam[e->cur], e->d_acc, e->idBase, (int)e->n);
    }
    HIP_TRY(hipGetLastError());
    e->aosValid = true;
    return SPH_OK;
}

// Table of the sampled-curve shapes for k_obb_ext, re-uploaded only when its inputs change.
int ensure_shape_table(SphEngine* e) {
    const SphParams& p = e->params;
    const float key[8] = {(float)p.param_shapeType, p.param_boxHalf[0], p.param_boxHalf[1], p.param_boxHalf[2],
                          p.param_shapeAux[0], p.param_shapeAux[1], p.param_shapeAux[2], 1.0f};
    if (e->d_shapeTab && std::memcmp(key, e->shapeKey, sizeof(key)) == 0) return SPH_OK;
    int rc;
    if (!e->d_shapeTab && (rc = dev_alloc(&e->d_shapeTab, 128))) return rc;
    float pts[384], b0[3];
    const int cnt = shape_table(p, pts, b0);
    float4 host[128];
    for (int i = 0; i < cnt; ++i) host[i] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], 0.0f);
    if (cnt) {
        // rare (parameter change): a synchronous copy keeps the pageable staging array safe
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(e->d_shapeTab, host, sizeof(float4) * (size_t)cnt, hipMemcpyHostToDevice));
    }
    e->shapeTab = sph::ShapeTab{e->d_shapeTab, cnt, b0[0], b0[1], b0[2]};
    std::memcpy(e->shapeKey, key, sizeof(key));
    return SPH_OK;
}

// boundaryFirst (z-slab engines, sph_slab_step_begin): the SPH pass runs the slot ranges next to the slab's faces first and
// records e->evBoundary behind them, so that the pack of the next exchange can start while the interior is computed.
int dispatch_one(SphEngine* e, float overrideDt, bool boundaryFirst = false) {
    if (e->params.param_pause) { if (boundaryFirst) HIP_TRY(hipEventRecord(e->evBoundary, e->stream)); return SPH_OK; }                               // SPHFluid3D.cpp:432
    int rc;
    if (e->trM && (rc = needs_sorted_copy(e, "tracers need"))) return rc;
    if (e->scK && (rc = needs_sorted_copy(e, "scalars need"))) return rc;
    if (e->dfC && (rc = needs_sorted_copy(e, "diffuse particles need"))) return rc;
    if (e->gtTab.count && (rc = needs_sorted_copy(e, "gates need"))) return rc;
    if (e->monCount && (rc = needs_sorted_copy(e, "monitors need"))) return rc;
    if ((rc = validate_params(e->params)) || (rc = couple_refused(e))) return rc;
    float cont[15];
    container_key(e->params, cont);
    const bool sameContainer = std::memcmp(cont, e->lastContainer, sizeof(cont)) == 0;   // same walls and same grid as the dispatch before
    const float dt = overrideDt > 0.0f ? overrideDt : e->params.param_timeStep;   // :434
    e->lastDt = dt;
    compute_grid_extents(e->params, e->grid);                               // :439
    if ((rc = ensure_grid_buffers(e))) return rc;                           // :440-447
    SimK k;
    make_simk(e->params, e->grid, dt, k);
    if (e->dfC && e->dfCrOn) {                                              // (refused before anything is launched)
        float radius = 0.0f;
        int stencil = 0;
        if (!diffuse_crest_args(e, k.cellSize, &radius, &stencil))
            return fail(SPH_ERR_STATE, "diffuse crest radius %g is above three cells (%g) of this grid", (double)radius, (double)(3.0f * k.cellSize));
    }
    if (e->slab) {
        if (e->z1 > e->grid.dims[2] || e->z0 < 0) return fail(SPH_ERR_STATE, "slab [%d,%d) outside the %d-layer grid", e->z0, e->z1, e->grid.dims[2]);
        k.gz = e->z1 - e->z0 + 2; k.numCells = k.gx * k.gy * k.gz; k.zoff = e->z0 - 1;
        // the pack that follows this substep may restrict itself to the ends of the slot range (same container as the substep
        // before, sorted slots): a particle that this substep carries from the middle into a face layer is then reported
        if (e->optGridBuild != 1 && sameContainer) k.slabFlags = e->d_slabCnt + kSlabCntFlags;
    }
    if ((rc = import_state(e))) return rc;
    const int n = (int)(e->slab ? e->nSlots : e->n);
    StateIn in{e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur]};
    const int nx = e->cur ^ 1;
    if (k.obbDeferred && (rc = ensure_shape_table(e))) return rc;
    // the array is current: keep it current from the SPH pass (not when OBB runs as its own pass afterwards)
    const bool fuseAos = !e->slab && e->optAos == 0 && e->aosValid && !k.obbDeferred && !e->obsK && !e->cpBuoy;   // (nor when obstacles or the buoyancy kick act afterwards)
    StateOut out{e->d_pos[nx], e->d_vel[nx], e->d_rp[nx], e->d_foam[nx], e->d_acc, fuseAos ? e->d_aos : nullptr, e->idBase};
    if (e->optGridBuild == 1) {
        // ---- A/B variant: the reference's atomicExchange linked lists (no sorting) ----
        if (e->slab) return fail(SPH_ERR_STATE, "the linked-list variant is single-GPU only");
        if (!e->d_llNext) {
            if ((rc = dev_alloc(&e->d_llNext, e->cap)) || (rc = dev_alloc(&e->d_llCell, e->cap)) || (rc = dev_alloc(&e->d_llKey, e->cap))) return rc;
        }
        int32_t* cellHead = reinterpret_cast<int32_t*>(e->d_cellStart);      // C+1 ints, reused as cellHead
        {
            Timed t(e, SPH_K_SCAN);
            hipLaunchKernelGGL(k_ll_clear, dim3(blocks_for((size_t)k.numCells)), dim3(kBlock), 0, e->stream, cellHead, k.numCells);
        }
        if (n) {
            {
                Timed t(e, SPH_K_BIN);
                hipLaunchKernelGGL(k_ll_build, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, in.pos, cellHead, e->d_llNext, e->d_llCell, e->d_llKey, n);
            }
            Timed t(e, SPH_K_SPH);
            hipLaunchKernelGGL(k_sph_ll, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, in, out, cellHead, e->d_llNext, n);
        }
    } else {
    if ((rc = build_grid(e, k, true))) return rc;                           // :449-468
    if (e->trM && (rc = tracers_advect(e, k, dt))) return rc;               // (reads the sorted copy and cellStart, as the SPH pass does)
    if (e->monCount && (rc = monitors_step(e, k, dt))) return rc;           // (the same two; DESIGN.md section 3s: a probe of the entry state)
    if (e->dfC && (rc = diffuse_step(e, k, dt, (uint32_t)n))) return rc;    // (the same two, and the sorted own data)
    if (e->scK && (rc = scalars_step(e, k, dt))) return rc;                 // (the same two, and the sorted own data)
    if (n) {                                                                // :470-509 (SPH + OBB fused)
        if (!e->d_sPV || e->sortedCap < (size_t)n) return fail(SPH_ERR_STATE, "sorted copy missing");
        const uint32_t* live = e->slab ? e->d_cellStart + k.numCells : nullptr;
        SortedIn S{e->d_sPV, e->d_sOwn};
        Timed t(e, SPH_K_SPH);
        if (e->optNeighbor >= 3 && (size_t)n < ((size_t)1 << 27)) {        // (buffer loads address the sorted copy with 32-bit byte offsets)
            const dim3 grid(8 * ((blocks_for(n, 256) + 7) / 8));
            auto walk = [&](hipStream_t st, const uint32_t* lo, const uint32_t* hi, bool bothEnds = false) {
                const int dbg = (e->debugFlags & ~256) | (bothEnds ? 256 : 0);    // (bit 8: the launch covers [0, *lo) and [*hi, end) instead of [*lo, *hi))
                if (k.h2 <= 1.0f)
                    hipLaunchKernelGGL((k_sph_walk<SPH_WALK_MAXN, SPH_WALK_UNROLL, SPH_WALK_CAP, true>), grid, dim3(256), 0, st, k, S, in, out,
                                       e->d_order, e->d_cellStart, live, n, dbg, e->d_stats, lo, hi);
                else
                    hipLaunchKernelGGL((k_sph_walk<SPH_WALK_MAXN, SPH_WALK_UNROLL, SPH_WALK_CAP, false>), grid, dim3(256), 0, st, k, S, in, out,
                                       e->d_order, e->d_cellStart, live, n, dbg, e->d_stats, lo, hi);
            };
            // The pack of the next exchange only reads the slots of the kSlabDepth lowest / highest local cell layers (k_slab_pack,
            // under the same conditions): those two slot ranges first, the event, then everything in between.
            const bool split = boundaryFirst && e->slab && k.gz > 2 * kSlabDepth && !k.obbDeferred && sameContainer;
            const bool timedStep = boundaryFirst && e->optTiming && e->evPassEnd;
            if (split) {
                const uint32_t* endLo = e->d_cellStart + kSlabDepth * (size_t)(k.gx * k.gy);
                const uint32_t* startHi = e->d_cellStart + (size_t)(k.gz - kSlabDepth) * (size_t)(k.gx * k.gy);
                // Both face ranges go FIRST, as ONE launch on the engine's stream (one tail instead of two) -- the exchange behind them needs them
                // early: the transfer has to fit beside the interior -- and the interior goes to a LOW-priority stream of its own that starts
                // with the face launch: beside it and, later, beside the pack / unpack kernels of the high-priority exchange stream, it fills
                // whatever they leave free.  Same inputs, disjoint output slots; the engine's stream joins the interior at the end of the pass.
                // Measured schedules (one rank's share of configs[4], bench.py --slab-path): this one 1.313-1.316 ms per substep; two face
                // launches + interior behind the first 1.351-1.355; merged faces + interior behind them 1.348-1.354
                // (profiles/r03_slab_face_launch_schedules.txt, profiles/r04_slab_face_launch_schedules.txt).
                HIP_TRY(hipEventRecord(e->evSorted, e->stream));
                walk(e->stream, endLo, startHi, true);
                HIP_TRY(hipEventRecord(e->evBoundary, e->stream));
                HIP_TRY(hipStreamWaitEvent(e->bstream, e->evSorted, 0));
                walk(e->bstream, endLo, startHi);
                HIP_TRY(hipEventRecord(e->evInterior, e->bstream));
                boundaryFirst = false;                                     // recorded
                HIP_TRY(hipStreamWaitEvent(e->stream, e->evInterior, 0));
            } else {
                walk(e->stream, nullptr, nullptr);
            }
            if (timedStep) HIP_TRY(hipEventRecord(e->evPassEnd, e->stream));
        } else if (e->optNeighbor >= 2) {
            hipLaunchKernelGGL((k_sph_list<SPH_LIST_MAXN, SPH_LIST_UNROLL, SPH_LIST_CAP>), dim3(8 * ((blocks_for(n, SPH_LIST_BLOCK) + 7) / 8)), dim3(SPH_LIST_BLOCK), 0, e->stream, k, S, in, out,
                               e->d_order, e->d_cellStart, live, n, e->debugFlags, e->d_stats);
        } else {
            hipLaunchKernelGGL(k_sph_slow, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, S, in, out, e->d_order, e->d_cellStart, n);
        }
    }
    }
    if (n && k.obbDeferred) {                                               // :495-509 for shapes 7..14
        Timed t(e, SPH_K_OTHER);
        const uint32_t* live = (e->slab && e->optGridBuild != 1) ? e->d_cellStart + k.numCells : nullptr;
        hipLaunchKernelGGL(k_obb_ext, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, e->shapeTab, out.pos, out.vel, live, n,
                           (e->slab && e->optGridBuild != 1) ? (const float4*)e->d_sOwn : (const float4*)nullptr);
    }
    if (e->obsK && (rc = obstacles_step(e, out.pos, out.vel, n, dt))) return rc;   // (after the container, before river / fountain)
    if (e->scK && (e->cpBuoy || e->cpTab.nSrc) && (rc = couple_step(e, out.pos, out.vel, n, dt))) return rc;   // (sources, then buoyancy)
    if (e->gtTab.count && (rc = gates_step(e, out.pos, out.vel, n, dt))) return rc;   // (sees the kick's velocity and the sources' values)
    const bool riverOn = e->river.riverMode && !e->terrainHeights.empty();   // :512
    if (riverOn) {                                                           // :511-516, DispatchTerrainConstraints / ChannelConstraint / StreamEmit
        if (e->slab) return fail(SPH_ERR_STATE, "riverMode on a z-slab engine: recycled particles jump across slabs (single-GPU engines only)");
        if (n) {
            const SphParams& p = e->params;
            const SphRiver& r = e->river;
            RiverK rk{r.terrainW, r.terrainH, r.terrainWorldMinX, r.terrainWorldMinZ, r.terrainWorldSizeX, r.terrainWorldSizeZ,
                      0.02f, 1.0f - 0.05f, p.param_boxCenter[0], r.riverAmp, r.riverFreq, r.riverPhase, r.riverChannelWidth,
                      80.0f, p.param_timeStep, r.riverSinkY, r.riverSinkZMax, r.riverEmitterPos[0], r.riverEmitterPos[1], r.riverEmitterPos[2],
                      r.riverEmitterVel[0], r.riverEmitterVel[1], r.riverEmitterVel[2], r.riverEmitterRadius,
                      r.riverSinkZMax - r.riverEmitterPos[2], p.param_restDensity};
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_river, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, rk, e->d_terrain, out.pos, out.vel, out.rp,
                               fuseAos ? (float4*)nullptr : e->d_acc, fuseAos ? e->d_aos : (SphParticle*)nullptr, e->d_aos, e->idBase, n);
        }
    }
    if (e->fountain.fountainMode && !e->river.riverMode) {                  // :519, :526-544
        if (e->slab) return fail(SPH_ERR_STATE, "fountainMode on a z-slab engine: recycled particles jump across slabs (single-GPU engines only)");
        if (n) {
            float half[3];
            effective_half(e->params, half);
            const SphParams& p = e->params;
            const SphFountain& f = e->fountain;
            FountainK fk{p.param_boxCenter[0] + f.fountainOffset[0], p.param_boxCenter[1] + f.fountainOffset[1],
                         p.param_boxCenter[2] + f.fountainOffset[2], f.fountainRadius, f.fountainSpread, f.fountainJetSpeedLive,
                         (p.param_boxCenter[1] - half[1]) + f.fountainDrainLevel, std::fmin(1.0f, f.fountainDrainPerSec * dt),
                         p.param_restDensity, f.fountainSeed * 747796405u};
            Timed t(e, SPH_K_OTHER);
            const uint32_t* live = (e->slab && e->optGridBuild != 1) ? e->d_cellStart + k.numCells : nullptr;
            hipLaunchKernelGGL(k_fountain, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, fk, out.pos, out.vel, out.rp,
                               fuseAos ? (float4*)nullptr : e->d_acc, fuseAos ? e->d_aos : (SphParticle*)nullptr, e->idBase, live, n);
        }
        e->fountain.fountainSeed++;
    }
    HIP_TRY(hipGetLastError());
    if (boundaryFirst) HIP_TRY(hipEventRecord(e->evBoundary, e->stream));   // no split launch: the pack waits for the whole pass
    e->cur = nx;
    e->accValid = !fuseAos;
    e->aosValid = fuseAos;
    if (e->slab) {   // the sorted output holds exactly the live particles: their count is on the device (kSlabCntLive)
        const bool sorted = e->optGridBuild != 1 && n > 0;
        if (!sorted) HIP_TRY(hipMemcpyAsync(e->d_slabCnt + kSlabCntLive, e->d_cellStart + k.numCells, sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream));   // (k_rank stored it otherwise)
        // the next k_slab_pack may restrict itself to the ends of the slot range if this substep cannot have moved a
        // particle by more than one layer: a container that did not change under the fluid (and the SPH pass reports the particle that
        // jumps from the middle into a face layer all the same, slab_check_layer_move)
        if (!sameContainer) slab_hold(e);                    // the walls moved under the fluid: whole faces until the counts have been seen calm again
        std::memcpy(e->lastContainer, cont, sizeof(cont));
        e->slabOrderValid = sorted && sameContainer;
        return SPH_OK;
    }
    if (e->optAos == 0 && !e->aosValid) return writeback(e);
    return SPH_OK;
}

}  // namespace

namespace {
using namespace sph;

// What the unpack kernels need to tell whether a received particle respects the exchange's one-layer assumption.
SlabGeom slab_geom(SphEngine* e) {
    sph::compute_grid_extents(e->params, e->grid);
    SlabGeom g;
    g.gminz = e->grid.gridMin[2]; g.cellSize = e->grid.cellSize; g.gzGlobal = e->grid.dims[2];
    g.z0 = e->z0; g.z1 = e->z1; g.hasLo = e->hasLo; g.hasHi = e->hasHi;
    return g;
}

// The preamble of the sph_slab_* entry points: an engine, a slab engine, and where the call moves faces one that has them.
int slab_engine(const SphEngine* e, bool needFaces = false) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (needFaces) return e->slab && e->d_face[0] ? SPH_OK : fail(SPH_ERR_STATE, "slab engine with face buffers required");
    return e->slab ? SPH_OK : fail(SPH_ERR_STATE, "not a slab engine");
}

// Device-side error flags of the exchange (kSlabCntFlags) as a status: every entry point that synchronises anyway reports them.
int slab_flags_error(const SphEngine* e, uint32_t flags, uint32_t nLo, uint32_t nHi) {
    if (flags & SPH_SLAB_FLAG_SEND_OVERFLOW) return fail(SPH_ERR_CAPACITY, "halo send buffer overflowed (%u / %u records for a capacity of %u)", nLo, nHi, e->faceCap);
    if (flags & SPH_SLAB_FLAG_SLOT_OVERFLOW) return fail(SPH_ERR_CAPACITY, "slab capacity %zu exceeded while appending halo records", e->cap);
    if (flags & SPH_SLAB_FLAG_BAD_HEADER) return fail(SPH_ERR_HIP, "a received halo message did not start with a valid header (magic / count): failed or garbled receive");
    if (flags & SPH_SLAB_FLAG_TRUNCATED) return fail(SPH_ERR_CAPACITY, "a neighbour rank had more halo records than its message could carry (face capacity %u)", e->faceCap);
    if (flags & SPH_SLAB_FLAG_SIZE_MISMATCH) return fail(SPH_ERR_STATE, "the two ends of a link sized an exchange's messages differently (a received header names other message sizes than this engine received): "
                                                "the ranks' call sequences differ");
    // (SPH_SLAB_FLAG_LAYER_JUMP -- a particle crossed more cell layers in z within one substep than the exchange follows -- loses nothing: it is a notice
    //  that the decomposed run no longer equals the single-domain run, carried by sph_slab_status's out[4], cleared by sph_slab_clear_flags)
    return SPH_OK;
}

template <class K>
int launch_impulse(SphEngine* e, const K& kk) {
    int rc;
    if ((rc = import_state(e))) return rc;
    const size_t nw = e->slab ? e->nSlots : e->n;
    if (e->slab) slab_hold(e);                              // (z-slabs: an impulse may set a face's record count moving: whole faces for three exchanges)
    if (nw) {
        Timed t(e, SPH_K_IMPULSE);
        hipLaunchKernelGGL((k_impulse<K>), dim3(blocks_for(nw)), dim3(kBlock), 0, e->stream, kk, e->d_pos[e->cur], e->d_vel[e->cur],
                           (e->aosValid && !e->slab) ? e->d_aos : nullptr, e->idBase, (int)nw);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}
}  // namespace

// ======================================================================== C-ABI
extern "C" {

int sph_abi_version(void) { return SPH_ABI_VERSION; }
const char* sph_last_error(void) { return g_err.c_str(); }

int sph_params_default(SphParams* out) {
    if (!out) return fail(SPH_ERR_ARG, "null params");
    sph::params_default(*out);
    return SPH_OK;
}
int sph_rotation_mat3(const float eulerDeg[3], float outM[9]) {
    if (!eulerDeg || !outM) return fail(SPH_ERR_ARG, "null argument");
    sph::rotation_mat3(eulerDeg, outM);
    return SPH_OK;
}
int sph_effective_half(const SphParams* params, float outHalf[3]) {
    if (!params || !outHalf) return fail(SPH_ERR_ARG, "null argument");
    sph::effective_half(*params, outHalf);
    return SPH_OK;
}
int sph_compute_grid_extents(const SphParams* params, SphGridInfo* out) {
    if (!params || !out) return fail(SPH_ERR_ARG, "null argument");
    sph::compute_grid_extents(*params, *out);
    return SPH_OK;
}
int sph_spawn_particles(const SphParams* params, size_t nRequested, uint32_t seed, SphParticle* out, size_t* nOut, float* massOut) {
    if (!params || !out || !nOut || !massOut) return fail(SPH_ERR_ARG, "null argument");
    std::vector<SphParticle> v;
    float m;
    sph::spawn_particles(*params, nRequested, seed, v, m);
    std::memcpy(out, v.data(), v.size() * sizeof(SphParticle));
    *nOut = v.size();
    *massOut = m;
    return SPH_OK;
}

static int create_common(SphEngine** out, const SphParams* params, void* stream, SphEngine** made) {
    if (!out || !params) return fail(SPH_ERR_ARG, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = validate_params(*params))) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(SPH_ERR_HIP, "no HIP device: this engine has no CPU fallback");
    SphEngine* e = new SphEngine();
    volumes_unbind_all(e);
    sph_fountain_default(&e->fountain);
    sph_river_default(&e->river);
    e->params = *params;
    if (stream) { e->stream = (hipStream_t)stream; e->ownStream = false; }
    else {
        hipError_t er = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
        if (er != hipSuccess) { delete e; return fail(SPH_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(er)); }
        e->ownStream = true;
    }
    *made = e;
    { std::lock_guard<std::mutex> lk(g_enginesMutex); g_engines.insert(e); }
    return SPH_OK;
}

int sph_create(SphEngine** out, size_t nRequested, const SphParams* params, uint32_t seed, void* stream) {
    SphEngine* e = nullptr;
    int rc = create_common(out, params, stream, &e);
    if (rc) return rc;
    std::vector<SphParticle> v;
    float m;
    sph::spawn_particles(e->params, nRequested, seed, v, m);          // SPHFluid3D.cpp:50
    e->params.param_mass = m;                                         // :92
    sph::compute_grid_extents(e->params, e->grid);                    // :53
    if ((rc = set_particles(e, v.data(), v.size())) || (rc = ensure_grid_buffers(e))) { sph_destroy(e); return rc; }
    *out = e;
    return SPH_OK;
}

int sph_create_from_particles(SphEngine** out, const SphParticle* particles, size_t n, const SphParams* params, void* stream) {
    if (!particles && n) return fail(SPH_ERR_ARG, "null particles");
    SphEngine* e = nullptr;
    int rc = create_common(out, params, stream, &e);
    if (rc) return rc;
    sph::compute_grid_extents(e->params, e->grid);
    if ((rc = set_particles(e, particles, n)) || (rc = ensure_grid_buffers(e))) { sph_destroy(e); return rc; }
    *out = e;
    return SPH_OK;
}

int sph_destroy(SphEngine* e) {
    if (!e) return SPH_OK;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->xstream) (void)hipStreamSynchronize(e->xstream);
    if (e->bstream) (void)hipStreamSynchronize(e->bstream);
    free_particle_buffers(e);
    free_grid_buffers(e);
    dev_free(e->d_dbg);
    dev_free(e->d_stencil);
    dev_free(e->d_terrain);
    dev_free(e->d_stats);
    sample_free(e);
    neighbors_free(e);
    components_free(e);
    knn_free(e);
    rays_free(e);
    shell_free(e);
    aniso_free(e);
    aggregate_free(e);
    surface_free(e);
    stats_free(e);
    tracers_free(e);
    diffuse_free(e);
    scalars_free(e);
    gates_free(e);
    monitors_free(e);
    obstacles_free(e);
    volumes_free(e);
    e->d_stateAcc.release();
    for (auto& ev : e->evLive) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto& ev : e->evPool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (e->xstream) { (void)hipStreamSynchronize(e->xstream); (void)hipStreamDestroy(e->xstream); }
    if (e->bstream) { (void)hipStreamSynchronize(e->bstream); (void)hipStreamDestroy(e->bstream); }
    {
        std::lock_guard<std::mutex> lk(g_enginesMutex);
        for (SphEngine* o : g_engines)                                        // a neighbour engine of this process must not wait for an event that is gone
            for (auto& pd : o->peerDone) if (pd && pd == e->evDone) pd = nullptr;
        g_engines.erase(e);
    }
    for (hipEvent_t ev : {e->evBoundary, e->evPacked, e->evDone, e->evSorted, e->evInterior, e->evPassEnd}) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->evX) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->evCnt) if (ev) (void)hipEventDestroy(ev);
    if (e->h_seen) (void)hipHostFree(e->h_seen);
    if (e->hstream) { (void)hipStreamSynchronize(e->hstream); (void)hipStreamDestroy(e->hstream); }
    if (e->evIntent) (void)hipEventDestroy(e->evIntent);
    if (e->h_intent) (void)hipHostFree(e->h_intent);
    dev_free(e->d_intent);
    if (e->ownStream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return SPH_OK;
}

int sph_reset(SphEngine* e, size_t nRequested, uint32_t seed) {       // SPHFluid3D.cpp:713-731
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = validate_params(e->params))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->surfValid = false;                                             // (the borrowed surface arrays end here: sph_abi.h)
    neighbors_free(e);                                                // (and the neighbour lists)
    components_free(e);                                               // (and the components)
    knn_free(e);                                                      // (and the k nearest neighbours)
    rays_free(e);                                                     // (and the ray hits and spans)
    shell_free(e);                                                    // (and the free-surface rows)
    aniso_free(e);                                                    // (and the anisotropy rows)
    aggregate_free(e);                                                // (and the stage of the neighbourhood reductions)
    tracers_free(e);                                                  // (and the tracer set)
    diffuse_free(e);                                                  // (and the pool of diffuse particles)
    scalars_free(e);                                                  // (and the scalar channels)
    gates_free(e);                                                    // (and the flow gates)
    monitors_free(e);                                                 // (and every field monitor)
    if (e->d_obsAcc) HIP_TRY(hipMemsetAsync(e->d_obsAcc, 0, sizeof(sph::ObsAcc), e->stream));   // (obstacles: the set and the poses stay, the sums restart)
    std::vector<SphParticle> v;
    float m;
    if (e->river.riverMode && !e->terrainHeights.empty())             // :104
        sph::spawn_river_particles(e->params, e->river, e->terrainHeights.data(), nRequested, seed, v, m);
    else
        sph::spawn_particles(e->params, nRequested, seed, v, m);
    e->params.param_mass = m;
    sph::compute_grid_extents(e->params, e->grid);
    free_particle_buffers(e);                                         // :714-719 delete + recreate
    if ((rc = set_particles(e, v.data(), v.size()))) return rc;
    return ensure_grid_buffers(e);
}

int sph_set_params(SphEngine* e, const SphParams* params) {
    if (!e || !params) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_params(*params))) return rc;
    e->params = *params;
    return SPH_OK;
}
int sph_get_params(const SphEngine* e, SphParams* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->params;
    return SPH_OK;
}
int sph_set_option(SphEngine* e, int option, int value) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    switch (option) {
    case SPH_OPT_NEIGHBOR_KERNEL: if (value < 1 || value > 3) return fail(SPH_ERR_ARG, "SPH pass %d: 3 = k_sph_walk, 2 = k_sph_list, 1 = k_sph_slow (0, the round-1 LDS tile pass, and 4, round 4's k_sph_tile, were retired)", value); e->optNeighbor = value; break;
    case SPH_OPT_GRID_BUILD: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optGridBuild = value; break;
    case SPH_OPT_AOS_MODE: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optAos = value; break;
    case SPH_OPT_TIMING: if (value < 0 || value > 2) return fail(SPH_ERR_ARG, "bad value"); e->optTiming = value; break;
    case SPH_OPT_GRAPH: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optGraph = value; break;
    case SPH_OPT_MESH_SPLIT: if (value < 0 || value > 64) return fail(SPH_ERR_ARG, "bad value"); e->optMeshSplit = value; break;
    case SPH_OPT_SCALAR_SWEEP: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optScalarSweep = value; break;
    case SPH_OPT_DIFFUSE_TIMED: if (value < 0 || value > 2) return fail(SPH_ERR_ARG, "bad value"); e->optDiffuseTimed = value; break;
    case SPH_OPT_NEIGHBORS_FILL: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optNbFill = value; break;
    case SPH_OPT_COMPONENTS_VARIANT: if (value < 0 || value > 3) return fail(SPH_ERR_ARG, "bad value"); e->optCcVariant = value; break;
    case SPH_OPT_KNN_VARIANT: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optKnnVariant = value; break;
    case SPH_OPT_RAYS_VARIANT: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optRaysVariant = value; break;
    case SPH_OPT_RAY_SPANS_VARIANT: if (value < 0 || value > 1) return fail(SPH_ERR_ARG, "bad value"); e->optRaySpansVariant = value; break;
    case SPH_OPT_AGGREGATE_VARIANT: if (value < 0 || value > 15) return fail(SPH_ERR_ARG, "bad value"); e->optAggVariant = value; break;
    case SPH_OPT_SHELL_TIMED: if (value < 0 || value > 3) return fail(SPH_ERR_ARG, "bad value"); e->optShellTimed = value; break;
    case SPH_OPT_DEBUG:
        e->debugFlags = value;
        if ((value & 8) && !e->d_stats) {
            int rc;
            if ((rc = dev_alloc(&e->d_stats, 8))) return rc;
            HIP_TRY(hipMemsetAsync(e->d_stats, 0, 8 * sizeof(unsigned long long), e->stream));
        }
        break;
    default: return fail(SPH_ERR_ARG, "unknown option %d", option);
    }
    return SPH_OK;
}
int sph_get_option(const SphEngine* e, int option, int* value) {
    if (!e || !value) return fail(SPH_ERR_ARG, "null argument");
    switch (option) {
    case SPH_OPT_NEIGHBOR_KERNEL: *value = e->optNeighbor; break;
    case SPH_OPT_GRID_BUILD: *value = e->optGridBuild; break;
    case SPH_OPT_AOS_MODE: *value = e->optAos; break;
    case SPH_OPT_TIMING: *value = e->optTiming; break;
    case SPH_OPT_GRAPH: *value = e->optGraph; break;
    case SPH_OPT_MESH_SPLIT: *value = e->optMeshSplit; break;
    case SPH_OPT_SCALAR_SWEEP: *value = e->optScalarSweep; break;
    case SPH_OPT_DIFFUSE_TIMED: *value = e->optDiffuseTimed; break;
    case SPH_OPT_NEIGHBORS_FILL: *value = e->optNbFill; break;
    case SPH_OPT_COMPONENTS_VARIANT: *value = e->optCcVariant; break;
    case SPH_OPT_KNN_VARIANT: *value = e->optKnnVariant; break;
    case SPH_OPT_RAYS_VARIANT: *value = e->optRaysVariant; break;
    case SPH_OPT_RAY_SPANS_VARIANT: *value = e->optRaySpansVariant; break;
    case SPH_OPT_AGGREGATE_VARIANT: *value = e->optAggVariant; break;
    case SPH_OPT_SHELL_TIMED: *value = e->optShellTimed; break;
    case SPH_OPT_GRAPH_LAUNCHES: *value = (int)e->graphLaunches; break;
    case SPH_OPT_DEBUG: *value = e->debugFlags; break;
    default: return fail(SPH_ERR_ARG, "unknown option %d", option);
    }
    return SPH_OK;
}

int sph_dispatch(SphEngine* e, float overrideDt) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    return dispatch_one(e, overrideDt);
}
// Key material of one sph_dispatch_n call for the graph cache: everything a captured launch sequence bakes in
// (uniforms, options, every device buffer a kernel gets, host-side validity state).  A hit compares the whole material,
// not only its hash.
static std::vector<unsigned char> graph_material(const SphEngine* e, float dt, int n) {
    std::vector<unsigned char> m;
    auto add = [&](const void* p, size_t len) { const unsigned char* b = static_cast<const unsigned char*>(p); m.insert(m.end(), b, b + len); };
    add(&e->params, sizeof(e->params));
    add(&dt, sizeof(dt)); add(&n, sizeof(n));
    // (whether the 80-byte array is current on entry only shapes the launches of the eager mode: fused update or write-back)
    const int opts[8] = {e->optNeighbor, e->optGridBuild, e->optAos, e->cur, ((e->aosValid && e->optAos == 0) ? 1 : 0) | (e->accValid ? 2 : 0) | (e->internalValid ? 4 : 0),
                         (int)e->idBase, e->allocatedCells, 0};
    add(opts, sizeof(opts));
    const void* ptrs[19] = {e->d_aos, e->d_pos[0], e->d_pos[1], e->d_vel[0], e->d_vel[1], e->d_rp[0], e->d_rp[1], e->d_foam[0], e->d_foam[1], e->d_acc,
                            e->d_binKey, e->d_intent, e->d_order, e->d_tmp, e->d_cellCount, e->d_cellStart, e->d_blockSums, e->d_sPV, e->d_sOwn};
    add(ptrs, sizeof(ptrs));
    const void* more[3] = {e->d_llNext, e->d_shapeTab, e->d_stats};
    add(more, sizeof(more));
    const size_t sz[2] = {e->n, e->cap};
    add(sz, sizeof(sz));
    // tracers: a call with tracers is never served by a graph captured without them, with another set's buffers or another history layout
    const void* tr[4] = {e->d_trRec, e->d_trPerm, e->d_trRing, e->d_trState};
    add(tr, sizeof(tr));
    const uint64_t trv[4] = {(uint64_t)e->trM, (uint64_t)e->trIntegrator, e->trK, e->trS};
    add(trv, sizeof(trv));
    // diffuse particles: pool set, its capacity and every buffer the substep's kernels get; the coefficients and all counts are read from memory
    const void* df[11] = {e->d_dfPool, e->d_dfScratch, e->d_dfState, e->d_dfCoef.p, e->d_dfFlag, e->d_dfFlagStart, e->d_dfFlagSums, e->d_dfPart,
                          e->d_dfCnt.p, e->d_dfCntStart.p, e->d_dfCntSums.p};
    add(df, sizeof(df));
    add(&e->dfC, sizeof(e->dfC));
    // scalars: a call with scalars is never served by a graph captured without them or with another channel count; the coefficients are read from memory
    const void* sc[4] = {e->d_scVal, e->d_scSorted, e->d_scCoef.p, e->d_scState};
    add(sc, sizeof(sc));
    add(&e->scK, sizeof(e->scK));
    add(&e->optScalarSweep, sizeof(e->optScalarSweep));
    // active scalars: the buffers and which of the coupling kernels run; coefficients, sources and their count are read from memory
    const void* cp[3] = {e->d_cpTab.p, e->d_cpAcc, e->d_cpPart};
    add(cp, sizeof(cp));
    const int cpWhat = (e->cpBuoy ? 1 : 0) | (e->cpTab.nSrc > 0 ? 2 : 0);
    add(&cpWhat, sizeof(cpWhat));
    // obstacles: the buffers and the count (the kernels read the bodies from memory, so a later set / set_motion needs no new graph)
    const void* ob[3] = {e->d_obs.p, e->d_obsAcc, e->d_obsPart};
    add(ob, sizeof(ob));
    add(&e->obsK, sizeof(e->obsK));
    // volumes: the table's address and whether any body is bound (which of the two obstacle kernels runs); the bindings and the lattices are read from memory
    const void* vt = e->d_volTab.p;
    const int anyBound = e->volBound > 0 ? 1 : 0;
    add(&vt, sizeof(vt));
    add(&anyBound, sizeof(anyBound));
    // dynamic bodies: the records' address and which finish kernel runs; the records are read from memory
    const void* dy = e->d_dyn.p;
    const int anyDyn = e->dynCount > 0 ? 1 : 0;
    add(&dy, sizeof(dy));
    add(&anyDyn, sizeof(anyDyn));
    // crest births of the pool, only while the term is on (off: the material of before): every buffer its launches get and the shell pass's
    // launch arguments (radius, hence the stencil, offset, minCount, flags); rate, windows, align and every are read from memory
    if (e->dfC && e->dfCrOn) {
        const void* cr[10] = {e->d_dfCrCoef.p, e->d_dfCrState, e->d_dfCrNrm.p, e->d_dfCrFlag.p, e->dfCrScan.tileMax.p, e->d_dfCrPart.p, e->d_dfCrOffsets.p,
                              e->dfCrScan.tileSums.p, e->d_dfCrSlots.p, e->d_dfCrCrest.p};
        add(cr, sizeof(cr));
        add(&e->dfCrCfg.radius, sizeof(float));                       // (with the params above it fixes the radius in force and the stencil)
        add(&e->dfCrCfg.offset, sizeof(float)); add(&e->dfCrCfg.minCount, sizeof(uint32_t)); add(&e->dfCrCfg.flags, sizeof(int32_t));
    }
    // flow gates, only while gates are set (off: the material of before): the buffers of the two launches; table, count, history and stride are read from memory
    if (e->gtTab.count) {
        const void* gt[4] = {e->d_gtTab.p, e->d_gtAcc, e->d_gtPart.p, e->d_gtRing.p};
        add(gt, sizeof(gt));
        add(&e->gtRingCap, sizeof(e->gtRingCap));
    }
    // field monitors, only while one is set (off: the material of before): per slot the kind, M, a lattice's dims (the launch grid), the
    // buffers and the ring layout; every, stride, the counters, wetFraction, a lattice's origin and spacing are read from memory
    if (e->monCount) {
        for (const MonitorSlot& s : e->mon) {
            const void* mo[6] = {s.d_tab.p, s.d_points.p, s.d_perm.p, s.d_rows.p, s.d_ring.p, s.d_times.p};
            add(mo, sizeof(mo));
            const uint64_t mv[7] = {(uint64_t)s.kind, (uint64_t)s.m, (uint64_t)s.dims[0], (uint64_t)s.dims[1], (uint64_t)s.dims[2], s.tab.history, s.tab.ringPoints};
            add(mv, sizeof(mv));
        }
    }
    return m;
}
static uint64_t graph_hash(const std::vector<unsigned char>& m) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char b : m) { h ^= b; h *= 1099511628211ull; }
    return h ? h : 1;
}

int sph_dispatch_n(SphEngine* e, float overrideDt, int nSubsteps) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    // Scene0p runs up to 16 substeps per frame with unchanged members (Scene0p.cpp:1482-1494, :3720-3739);
    // at the default 50 000 particles that loop is launch-bound, so the second identical call is
    // captured into a hipGraph and replayed from then on.
    const bool graphable = e->optGraph && nSubsteps >= 2 && !e->slab && !e->optTiming && !e->debugFlags &&
                           !e->fountain.fountainMode && !e->river.riverMode && !e->params.param_pause && e->n > 0;
    SphEngine::GraphEntry* hit = nullptr;
    uint64_t key = 0;
    std::vector<unsigned char> material;
    if (graphable) {
        material = graph_material(e, overrideDt, nSubsteps);
        key = graph_hash(material);
        for (auto& g : e->graphs) if (g.key == key && g.material == material) { hit = &g; break; }
        if (hit && hit->exec) {
            int crc;
            if ((crc = couple_refused(e))) return crc;           // (a replay changes nothing either)
            sph::compute_grid_extents(e->params, e->grid);       // what an eager dispatch would have refreshed (sph_grid_info, RefreshGrid)
            if (e->trM) {                                        // the processing order is re-sorted between calls, never inside a graph
                int trc;
                SimK k;
                make_simk(e->params, e->grid, e->params.param_timeStep, k);
                if ((trc = tracers_order(e, k))) return trc;
                e->trSteps += (uint64_t)nSubsteps;               // (the replayed k_tracer_tick launches advance the device counter)
            }
            if (e->scK) e->scSteps += (uint64_t)nSubsteps;
            HIP_TRY(hipGraphLaunch(hit->exec, e->stream));
            e->cur = hit->postCur; e->aosValid = hit->postAos; e->accValid = hit->postAcc; e->internalValid = true;
            hit->lastUse = ++e->graphClock;
            ++e->graphLaunches;
            return SPH_OK;
        }
    }
    const bool capture = graphable && hit;                   // seen once, run eagerly then: every buffer exists
    if (capture && e->trM) {                                 // (as before a replay: the cell sort stays outside the graph)
        sph::compute_grid_extents(e->params, e->grid);
        int trc;
        if ((trc = ensure_grid_buffers(e))) return trc;
        SimK k;
        make_simk(e->params, e->grid, e->params.param_timeStep, k);
        if ((trc = tracers_order(e, k))) return trc;
    }
    if (capture) HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    e->capturing = capture;
    int rc = SPH_OK;
    for (int i = 0; i < nSubsteps && !rc; ++i) rc = dispatch_one(e, overrideDt);
    e->capturing = false;
    if (capture) {
        hipGraph_t graph = nullptr;
        hipError_t er = hipStreamEndCapture(e->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (er != hipSuccess) return fail(SPH_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(er));
        er = hipGraphInstantiate(&hit->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (er != hipSuccess) { hit->exec = nullptr; return fail(SPH_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(er)); }
        hit->postCur = e->cur; hit->postAos = e->aosValid; hit->postAcc = e->accValid;
        hit->lastUse = ++e->graphClock;
        ++e->graphCaptures;
        HIP_TRY(hipGraphLaunch(hit->exec, e->stream));
        ++e->graphLaunches;
        return SPH_OK;
    }
    if (rc) return rc;
    if (graphable) {                                         // first sighting: remember it (at most 8 entries, LRU)
        if (e->graphs.size() >= 8) {
            size_t v = 0;
            for (size_t i = 1; i < e->graphs.size(); ++i) if (e->graphs[i].lastUse < e->graphs[v].lastUse) v = i;
            if (e->graphs[v].exec) {
                HIP_TRY(hipStreamSynchronize(e->stream));
                (void)hipGraphExecDestroy(e->graphs[v].exec);
            }
            e->graphs.erase(e->graphs.begin() + (long)v);
        }
        SphEngine::GraphEntry g;
        g.key = key; g.material = material; g.lastUse = ++e->graphClock;
        e->graphs.push_back(g);
    }
    return SPH_OK;
}

int sph_apply_wave_impulse(SphEngine* e, float amplitude, float wavelength, float phase, const float dir[3], float yMin, float yMax) {
    if (!e || !dir) return fail(SPH_ERR_ARG, "null argument");
    if (amplitude == 0.0f || wavelength <= 1e-6f) return SPH_OK;      // SPHFluid3D.cpp:607
    int rc;
    if ((rc = import_state(e))) return rc;
    WaveK w;
    const float len = std::sqrt(std::fma(dir[2], dir[2], std::fma(dir[1], dir[1], dir[0] * dir[0])));
    if (len > 1e-6f) { w.ndx = dir[0] / len; w.ndy = dir[1] / len; w.ndz = dir[2] / len; }   // WaveImpulse.comp:39
    else { w.ndx = 0.0f; w.ndy = 1.0f; w.ndz = 0.0f; }
    w.amplitude = amplitude; w.kk = 6.28318530718f / wavelength; w.phase = phase; w.yMin = yMin; w.yMax = yMax;
    const size_t nw = e->slab ? e->nSlots : e->n;
    // z-slabs: a kick of A changes a particle's step by at most A dt, i.e. a face layer's record count by about A dt / h per substep: a gentle wave (the
    // scene's A = 1.5: 0.5 % of h per substep) leaves a calm face calm; anything that could outgrow the messages' margin within two exchanges holds them whole
    // (the dt that is actually stepped: the last dispatch's overrideDt if there was one)
    if (e->slab && std::fabs(amplitude) * (e->lastDt > 0.0f ? e->lastDt : e->params.param_timeStep) > 0.02f * e->params.param_h) slab_hold(e);
    if (nw) {
        Timed t(e, SPH_K_IMPULSE);
        hipLaunchKernelGGL(k_wave_impulse, dim3(blocks_for(nw)), dim3(kBlock), 0, e->stream, w, e->d_pos[e->cur], e->d_vel[e->cur],
                           (e->aosValid && !e->slab) ? e->d_aos : nullptr, e->idBase, (int)nw);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- per-frame impulses beyond WaveImpulse ------------------------

int sph_apply_vortex_impulse(SphEngine* e, float tangentKick, float inwardKick) {     // SPHFluid3D.cpp:627-646
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (std::fabs(tangentKick) < 1e-6f && std::fabs(inwardKick) < 1e-6f) return SPH_OK;
    float R[9], half[3];
    sph::rotation_mat3(e->params.param_boxEulerDeg, R);
    sph::effective_half(e->params, half);
    VortexK kk;
    kk.cx = e->params.param_boxCenter[0]; kk.cy = e->params.param_boxCenter[1]; kk.cz = e->params.param_boxCenter[2];
    kk.ax = R[3]; kk.ay = R[4]; kk.az = R[5];                                         // local +Y = column 1
    kk.tangent = tangentKick; kk.inward = inwardKick;
    kk.e1 = 0.35f * std::fmax(std::fmax(half[0], half[2]), 1e-4f);
    return launch_impulse(e, kk);
}

int sph_apply_attractor_impulse(SphEngine* e, const float point[3], float pullKick, float radius) {   // SPHFluid3D.cpp:650-664
    if (!e || !point) return fail(SPH_ERR_ARG, "null argument");
    if (std::fabs(pullKick) < 1e-6f) return SPH_OK;
    AttractorK kk;
    kk.px = point[0]; kk.py = point[1]; kk.pz = point[2];
    kk.radius = std::fmax(radius, 0.1f);
    kk.soften = std::fmax(0.15f * radius, 0.2f);
    kk.pullSoft = pullKick * kk.soften;
    kk.e0 = 0.6f * kk.radius;
    return launch_impulse(e, kk);
}

int sph_set_stencil_targets(SphEngine* e, const float* points4, size_t count) {       // SPHFluid3D.cpp:684-693
    if (!e || (!points4 && count)) return fail(SPH_ERR_ARG, "null argument");
    HIP_TRY(hipStreamSynchronize(e->stream));
    dev_free(e->d_stencil);
    e->stencilCount = 0;
    if (!count) return SPH_OK;
    int rc;
    if ((rc = dev_alloc(&e->d_stencil, count))) return rc;
    HIP_TRY(hipMemcpy(e->d_stencil, points4, count * sizeof(float4), hipMemcpyHostToDevice));
    e->stencilCount = count;
    return SPH_OK;
}

int sph_apply_stencil_attract(SphEngine* e, float pullKick, float dampKick) {         // SPHFluid3D.cpp:695-710
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->stencilCount == 0 || !e->d_stencil) return SPH_OK;
    if (std::fabs(pullKick) < 1e-6f && dampKick < 1e-6f) return SPH_OK;
    StencilK kk;
    kk.targets = e->d_stencil; kk.nTargets = (uint32_t)e->stencilCount;
    kk.pull = pullKick; kk.oneMinusDamp = 1.0f - std::fmin(dampKick, 0.5f);
    return launch_impulse(e, kk);
}

int sph_apply_curl_flow(SphEngine* e, float kick, float scale, float time) {          // SPHFluid3D.cpp:668-681
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (std::fabs(kick) < 1e-6f) return SPH_OK;
    CurlK kk;
    kk.kick = kick; kk.scale = std::fmax(scale, 1e-3f); kk.time = time;
    return launch_impulse(e, kk);
}

void sph_fountain_default(SphFountain* out) {               // SPHFluid3D.h:161-168
    if (!out) return;
    *out = SphFountain{0, {0.0f, -5.0f, 0.0f}, 1.0f, 0.25f, 25.0f, 1.0f, 2.0f, 0u};
}
int sph_set_fountain(SphEngine* e, const SphFountain* f) {
    if (!e || !f) return fail(SPH_ERR_ARG, "null argument");
    e->fountain = *f;
    return SPH_OK;
}
int sph_get_fountain(const SphEngine* e, SphFountain* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->fountain;
    return SPH_OK;
}

void sph_river_default(SphRiver* out) {                     // SPHFluid3D.h:171-196
    if (out) sph::river_default(*out);
}
static int validate_river(const SphRiver& r) {
    if (r.terrainW < 2 || r.terrainH < 2 || r.terrainW > 4096 || r.terrainH > 4096) return fail(SPH_ERR_ARG, "terrainW / terrainH %d x %d: 2..4096 each", r.terrainW, r.terrainH);
    return SPH_OK;
}
int sph_generate_river_terrain(SphParams* params, int seed, SphRiver* river, float* heights) {
    if (!params || !river || !heights) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_river(*river))) return rc;
    sph::river_terrain(*params, seed, *river, heights);
    return SPH_OK;
}
int sph_spawn_river_particles(const SphParams* params, const SphRiver* river, const float* heights, size_t nRequested, uint32_t seed,
                              SphParticle* out, size_t* nOut, float* massOut) {
    if (!params || !river || !heights || !out || !nOut || !massOut) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_river(*river))) return rc;
    std::vector<SphParticle> v;
    float m;
    sph::spawn_river_particles(*params, *river, heights, nRequested, seed, v, m);
    std::memcpy(out, v.data(), v.size() * sizeof(SphParticle));
    *nOut = v.size();
    *massOut = m;
    return SPH_OK;
}
int sph_set_river(SphEngine* e, const SphRiver* river, const float* heights) {
    if (!e || !river) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_river(*river))) return rc;
    const size_t cells = (size_t)river->terrainW * (size_t)river->terrainH;
    if (heights) {                                                   // :868-873
        for (size_t i = 0; i < cells; ++i) if (!std::isfinite(heights[i])) return fail(SPH_ERR_ARG, "terrain height %zu is not finite", i);
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (cells > e->terrainCap) {
            dev_free(e->d_terrain);
            e->terrainCap = 0;
            if ((rc = dev_alloc(&e->d_terrain, cells))) return rc;
            e->terrainCap = cells;
        }
        e->terrainHeights.assign(heights, heights + cells);
        HIP_TRY(hipMemcpy(e->d_terrain, heights, cells * sizeof(float), hipMemcpyHostToDevice));
    } else if (!e->terrainHeights.empty() && e->terrainHeights.size() != cells) {
        return fail(SPH_ERR_ARG, "terrainW x terrainH changed to %d x %d without a new heightfield", river->terrainW, river->terrainH);
    }
    e->river = *river;
    return SPH_OK;
}
int sph_get_river(const SphEngine* e, SphRiver* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->river;
    return SPH_OK;
}

size_t sph_num_particles(const SphEngine* e) { return e ? e->n : 0; }

int sph_grid_info(const SphEngine* e, SphGridInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->grid;
    return SPH_OK;
}

int sph_upload_particles(SphEngine* e, const SphParticle* host, size_t n) {
    if (!e || (!host && n)) return fail(SPH_ERR_ARG, "null argument");
    if (n != e->n) return fail(SPH_ERR_ARG, "upload of %zu records into an engine of %zu particles", n, e->n);
    if (n) HIP_TRY(hipMemcpyAsync(e->d_aos, host, n * sizeof(SphParticle), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->aosValid = true; e->internalValid = false; e->accValid = false;
    return SPH_OK;
}

int sph_download_particles(SphEngine* e, SphParticle* host, size_t n) {
    if (!e || (!host && n)) return fail(SPH_ERR_ARG, "null argument");
    if (n != e->n) return fail(SPH_ERR_ARG, "download of %zu records from an engine of %zu particles", n, e->n);
    int rc;
    if ((rc = writeback(e))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(host, e->d_aos, n * sizeof(SphParticle), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_device_particles(SphEngine* e, const SphParticle** devPtr) {
    if (!e || !devPtr) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = writeback(e))) return rc;
    *devPtr = e->d_aos;
    return SPH_OK;
}

int sph_pack_render_buffer(SphEngine* e, float* devOut4, size_t n, int wMode) {
    if (!e || (!devOut4 && n)) return fail(SPH_ERR_ARG, "null argument");
    if (e->slab) return fail(SPH_ERR_STATE, "a slab engine has no local 80-byte array");
    if (n != e->n) return fail(SPH_ERR_ARG, "size mismatch: %zu particles, engine has %zu", n, e->n);
    if (wMode < 0 || wMode > 4) return fail(SPH_ERR_ARG, "bad w mode %d", wMode);
    int rc;
    if ((rc = writeback(e))) return rc;
    if (n) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_pack_render, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, e->d_aos, reinterpret_cast<float4*>(devOut4), wMode, (int)n);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_initial_particles(const SphEngine* e, SphParticle* host, size_t n) {
    if (!e || (!host && n)) return fail(SPH_ERR_ARG, "null argument");
    if (n != e->hostInit.size()) return fail(SPH_ERR_ARG, "size mismatch");
    std::memcpy(host, e->hostInit.data(), n * sizeof(SphParticle));
    return SPH_OK;
}

int sph_download_grid(SphEngine* e, int32_t* cellCount, size_t nCells, int32_t* particleCell, size_t n) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    sph::compute_grid_extents(e->params, e->grid);
    if ((rc = ensure_grid_buffers(e))) return rc;
    if (nCells != (size_t)e->grid.numCells || n != e->n) return fail(SPH_ERR_ARG, "size mismatch (cells %d, particles %zu)", e->grid.numCells, e->n);
    SimK k;
    make_simk(e->params, e->grid, e->params.param_timeStep, k);
    if ((rc = import_state(e))) return rc;
    if ((rc = build_grid(e, k))) return rc;
    const size_t need = std::max(nCells, n);
    if (need > e->dbgCap) { dev_free(e->d_dbg); if ((rc = dev_alloc(&e->d_dbg, need))) return rc; e->dbgCap = need; }
    if (cellCount) {
        hipLaunchKernelGGL(k_debug_cells, dim3(blocks_for(nCells)), dim3(kBlock), 0, e->stream, e->d_cellStart, e->d_dbg, (int)nCells);
        HIP_TRY(hipMemcpyAsync(cellCount, e->d_dbg, nCells * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (particleCell && n) {
        hipLaunchKernelGGL(k_debug_particle_cell, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, e->d_pos[e->cur], e->d_vel[e->cur], e->d_dbg, e->idBase, (int)n);
        HIP_TRY(hipMemcpyAsync(particleCell, e->d_dbg, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_debug_counters(SphEngine* e, uint64_t* out, int count, int reset) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (count > 8) count = 8;
    for (int i = 0; i < count; ++i) out[i] = 0;
    if (!e->d_stats) return SPH_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long host[8];
    HIP_TRY(hipMemcpy(host, e->d_stats, sizeof(host), hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) out[i] = host[i];
    if (reset) HIP_TRY(hipMemset(e->d_stats, 0, sizeof(host)));
    return SPH_OK;
}

// ---- z-slab (multi-GPU) entry points -----------------------------------------------------------
int sph_create_slab(SphEngine** out, const SphParticle* particles, const uint32_t* ids, size_t n, const SphParams* params,
                    int z0, int z1, int hasLo, int hasHi, size_t capacity, void* stream) {
    if ((!particles || !ids) && n) return fail(SPH_ERR_ARG, "null particles / ids");
    if (z1 <= z0 || z0 < 0) return fail(SPH_ERR_ARG, "bad slab range [%d, %d)", z0, z1);
    if (capacity < n) return fail(SPH_ERR_ARG, "capacity %zu < %zu particles", capacity, n);
    if (hasLo && hasHi && z1 - z0 < 2)
        return fail(SPH_ERR_ARG, "an inner slab needs at least 2 cell layers (a migrant from below would have to become the upper neighbour's ghost within the same substep)");
    SphEngine* e = nullptr;
    int rc = create_common(out, params, stream, &e);
    if (rc) return rc;
    e->slab = true; e->z0 = z0; e->z1 = z1; e->hasLo = hasLo ? 1 : 0; e->hasHi = hasHi ? 1 : 0;
    sph::compute_grid_extents(e->params, e->grid);
    uint32_t* d_ids = nullptr;
    auto cleanup = [&](int code) { if (d_ids) (void)hipFree(d_ids); sph_destroy(e); return code; };
    if ((rc = alloc_particle_buffers(e, capacity))) return cleanup(rc);
    if ((rc = ensure_grid_buffers(e))) return cleanup(rc);
    e->n = n; e->nSlots = n;
    if (n) {
        if ((rc = dev_alloc(&d_ids, n))) return cleanup(rc);
        hipError_t er = hipMemcpyAsync(e->d_aos, particles, n * sizeof(SphParticle), hipMemcpyHostToDevice, e->stream);
        if (er == hipSuccess) er = hipMemcpyAsync(d_ids, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
        if (er != hipSuccess) return cleanup(fail(SPH_ERR_HIP, "upload failed: %s", hipGetErrorString(er)));
        hipLaunchKernelGGL(k_slab_import, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, e->d_aos, d_ids, e->d_pos[0], e->d_vel[0], e->d_rp[0], e->d_foam[0], (int)n);
    }
    uint32_t init[kSlabCounters] = {0u};
    init[kSlabCntLive] = (uint32_t)n;
    hipError_t er = hipMemcpyAsync(e->d_slabCnt, init, sizeof(init), hipMemcpyHostToDevice, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    if (er != hipSuccess) return cleanup(fail(SPH_ERR_HIP, "slab init failed: %s", hipGetErrorString(er)));
    if (d_ids) (void)hipFree(d_ids);
    e->cur = 0; e->internalValid = true; e->aosValid = false; e->accValid = false;
    *out = e;
    return SPH_OK;
}

int sph_slab_pack(SphEngine* e, void* sendLo, void* sendHi, uint32_t capLo, uint32_t capHi, uint32_t countsOut[2]) {
    if (!e || !countsOut) return fail(SPH_ERR_ARG, "null argument");
    if (int rc = slab_engine(e)) return rc;
    if ((e->hasLo && !sendLo) || (e->hasHi && !sendHi)) return fail(SPH_ERR_ARG, "missing send buffer");
    sph::compute_grid_extents(e->params, e->grid);
    SimK k;
    make_simk(e->params, e->grid, e->params.param_timeStep, k);
    HIP_TRY(hipMemsetAsync(e->d_slabCnt + kSlabCntRecLo, 0, 2 * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->d_slabCnt + kSlabCntPackedLo, 0, 2 * sizeof(uint32_t), e->stream));      // counts of an earlier async pack
    uint32_t host[kSlabCntLive + 1] = {0, 0, 0};              // RecLo, RecHi, Live
    // e->nSlots bounds the slots in use; the device-side live count (kSlabCntLive) trims it to the
    // slots that hold data, so no host round trip is needed before the launch
    if (e->nSlots) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL((k_slab_pack<false>), dim3(blocks_for(e->nSlots)), dim3(kBlock), 0, e->stream, k, e->z0, e->z1, e->hasLo, e->hasHi,
                           e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur], e->accValid ? e->d_acc : (const float4*)nullptr, (int)e->nSlots,
                           (SlabRec*)sendLo, (SlabRec*)sendHi, capLo, capHi, e->d_slabCnt,
                           slab_ranges_usable(e) ? e->d_cellStart : (const uint32_t*)nullptr, k.gx * k.gy);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, e->d_slabCnt, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->nSlots = std::min<size_t>(e->nSlots, host[kSlabCntLive]);
    const uint32_t nLo = host[kSlabCntRecLo], nHi = host[kSlabCntRecHi];
    // sph_slab_status adds Rec* and Packed*: the counts of this pack stay visible to it in Packed*, Rec* go back to zero
    HIP_TRY(hipMemsetAsync(e->d_slabCnt + kSlabCntRecLo, 0, 2 * sizeof(uint32_t), e->stream));
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_slabCnt + kSlabCntPackedLo, nLo);
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_slabCnt + kSlabCntPackedHi, nHi);
    HIP_TRY(hipGetLastError());
    if (nLo > capLo || nHi > capHi) return fail(SPH_ERR_CAPACITY, "halo send buffer too small (%u/%u lo, %u/%u hi)", nLo, capLo, nHi, capHi);
    countsOut[0] = nLo; countsOut[1] = nHi;
    return SPH_OK;
}

int sph_slab_unpack(SphEngine* e, const void* recvLo, uint32_t nLo, const void* recvHi, uint32_t nHi) {
    if (int rc = slab_engine(e)) return rc;
    if ((nLo && !recvLo) || (nHi && !recvHi)) return fail(SPH_ERR_ARG, "missing receive buffer");
    if (e->nSlots + nLo + nHi > e->cap) return fail(SPH_ERR_CAPACITY, "slab capacity %zu < %zu slots", e->cap, e->nSlots + nLo + nHi);
    const int c = e->cur;
    const SlabGeom geom = slab_geom(e);
    if (nLo) hipLaunchKernelGGL(k_slab_unpack, dim3(blocks_for(nLo)), dim3(kBlock), 0, e->stream, (const SlabRec*)recvLo, (int)nLo,
                                e->d_pos[c], e->d_vel[c], e->d_rp[c], e->d_foam[c], e->d_acc, (int)e->nSlots, geom, 1, e->d_slabCnt);
    e->nSlots += nLo;
    if (nHi) hipLaunchKernelGGL(k_slab_unpack, dim3(blocks_for(nHi)), dim3(kBlock), 0, e->stream, (const SlabRec*)recvHi, (int)nHi,
                                e->d_pos[c], e->d_vel[c], e->d_rp[c], e->d_foam[c], e->d_acc, (int)e->nSlots, geom, 0, e->d_slabCnt);
    e->nSlots += nHi;
    HIP_TRY(hipGetLastError());
    // until the next dispatch sorts again, every slot may hold data
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, e->stream, e->d_slabCnt + kSlabCntLive, (uint32_t)e->nSlots);
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_slab_download(SphEngine* e, void* hostOut, size_t capRecords, size_t* nOut) {
    if (!e || !nOut || (!hostOut && capRecords)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = slab_engine(e))) return rc;
    uint32_t cnts[kSlabCntPackedHi + 1] = {0};
    HIP_TRY(hipMemcpyAsync(cnts, e->d_slabCnt, sizeof(cnts), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->xstream) HIP_TRY(hipStreamSynchronize(e->xstream));
    // a face or slot overflow dropped records: the owned set would come back short without a word.  (SPH_SLAB_FLAG_LAYER_JUMP -- a particle crossed
    // more layers than the exchange follows -- drops nothing: the records are delivered, sph_slab_status carries the notice.)
    if ((rc = slab_flags_error(e, cnts[kSlabCntFlags], cnts[kSlabCntPackedLo], cnts[kSlabCntPackedHi]))) return rc;
    const size_t n = cnts[kSlabCntLive];
    SlabOut* d_out = nullptr;
    if ((rc = dev_alloc(&d_out, n ? n : 1))) return rc;
    hipError_t er = hipMemsetAsync(e->d_slabCnt + kSlabCntDownload, 0, sizeof(uint32_t), e->stream);
    if (er == hipSuccess && n)
        hipLaunchKernelGGL(k_slab_download, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur],
                           e->d_foam[e->cur], e->d_acc, (int)n, e->accValid ? 1 : 0, d_out, (uint32_t)n, e->d_slabCnt + kSlabCntDownload);
    uint32_t cnt = 0;
    if (er == hipSuccess) er = hipMemcpyAsync(&cnt, e->d_slabCnt + kSlabCntDownload, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    if (er == hipSuccess && cnt > capRecords) { (void)hipFree(d_out); return fail(SPH_ERR_CAPACITY, "%u owned records > capacity %zu", cnt, capRecords); }
    if (er == hipSuccess && cnt) er = hipMemcpy(hostOut, d_out, (size_t)cnt * sizeof(SlabOut), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (er != hipSuccess) return fail(SPH_ERR_HIP, "slab download failed: %s", hipGetErrorString(er));
    *nOut = cnt;
    return SPH_OK;
}

// ---- exchange without host round trips (device-side counts) + RCCL transport -------------------------------------
int sph_slab_alloc_faces(SphEngine* e, uint32_t faceCap) {
    int rc;
    if ((rc = slab_engine(e))) return rc;
    if (faceCap == 0) return fail(SPH_ERR_ARG, "face capacity must be > 0");
    if (e->faceCap == faceCap && e->d_face[0]) return SPH_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 4; ++i) {
        dev_free(e->d_face[i]);
        if ((rc = dev_alloc(&e->d_face[i], slab_face_bytes(faceCap)))) return rc;
        HIP_TRY(hipMemsetAsync(e->d_face[i], 0, sizeof(SlabHdr), e->stream));      // no header yet
    }
    if (!e->h_seen) {
        HIP_TRY(hipHostMalloc((void**)&e->h_seen, 4 * sizeof(SlabSeen), hipHostMallocDefault));
        for (auto& ev : e->evCnt) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    for (auto& v : e->cntValid) v = false;
    e->faceCap = faceCap;
    e->faceAgreedWith = nullptr;
    return SPH_OK;
}
int sph_slab_face_buffer(SphEngine* e, int which, void** devPtr) {
    if (!e || !devPtr) return fail(SPH_ERR_ARG, "null argument");
    if (which < 0 || which > 3 || !e->d_face[which]) return fail(SPH_ERR_STATE, "no face buffers: call sph_slab_alloc_faces first");
    *devPtr = e->d_face[which];
    return SPH_OK;
}
int sph_slab_face_bytes(SphEngine* e, uint64_t* bytes) {
    if (!e || !bytes) return fail(SPH_ERR_ARG, "null argument");
    if (!e->faceCap) return fail(SPH_ERR_STATE, "no face buffers: call sph_slab_alloc_faces first");
    *bytes = (uint64_t)slab_face_bytes(e->faceCap);
    return SPH_OK;
}
static SlabMsg slab_msg_whole(uint32_t faceCap) { return SlabMsg{{faceCap, faceCap}, {faceCap, faceCap}}; }   // whole faces
static void grid_key(const SphGridInfo& g, float out[8]) {
    const float v[8] = {g.gridMin[0], g.gridMin[1], g.gridMin[2], g.cellSize, (float)g.dims[0], (float)g.dims[1], (float)g.dims[2], 0.0f};
    std::memcpy(out, v, sizeof(v));
}
static int slab_pack_on(SphEngine* e, hipStream_t st) {
    if (int rc = slab_engine(e, true)) return rc;
    sph::compute_grid_extents(e->params, e->grid);
    SimK k;
    make_simk(e->params, e->grid, e->params.param_timeStep, k);
    grid_key(e->grid, e->packGrid);                         // the records this pack cuts are classified for THIS grid (sph_slab_step_begin checks it)
    e->packGridValid = true;
    e->nSlots = e->cap;                                     // from now on only a launch bound: kSlabCntLive counts the slots in use
    {                                                       // (the running counts HaloLo .. MigHi are zero: set at creation, reset by k_slab_headers2)
        Timed t(e, SPH_K_OTHER, st);
        hipLaunchKernelGGL((k_slab_pack<true>), dim3(blocks_for(e->cap)), dim3(kBlock), 0, st, k, e->z0, e->z1, e->hasLo, e->hasHi,
                           e->d_pos[e->cur], e->d_vel[e->cur], e->d_rp[e->cur], e->d_foam[e->cur], e->accValid ? e->d_acc : (const float4*)nullptr, (int)e->cap,
                           (SlabRec*)e->d_face[0], (SlabRec*)e->d_face[1], e->faceCap, e->faceCap, e->d_slabCnt,
                           slab_ranges_usable(e) ? e->d_cellStart : (const uint32_t*)nullptr, k.gx * k.gy);
        hipLaunchKernelGGL(k_slab_headers2, dim3(1), dim3(1), 0, st, e->d_slabCnt, e->hasLo ? e->d_face[0] : (char*)nullptr,
                           e->hasHi ? e->d_face[1] : (char*)nullptr, e->faceCap, e->msgSend);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}
// msg: records the messages carried; the face capacity when whole faces were moved
static int slab_unpack_on(SphEngine* e, hipStream_t st, const void* recvLo, const void* recvHi, uint32_t recvCap, const SlabMsg& msg) {
    if (int rc = slab_engine(e)) return rc;
    if (recvCap != e->faceCap || !e->faceCap) return fail(SPH_ERR_ARG, "received faces must have this engine's face capacity (%u, got %u)", e->faceCap, recvCap);
    const char* const face[2] = {e->hasLo ? (const char*)recvLo : nullptr, e->hasHi ? (const char*)recvHi : nullptr};
    if ((e->hasLo && !face[0]) || (e->hasHi && !face[1])) return fail(SPH_ERR_ARG, "missing receive buffer");
    const int c = e->cur;
    e->nSlots = e->cap;
    const SlabGeom geom = slab_geom(e);
    Timed t(e, SPH_K_OTHER, st);
    for (int d = 0; d < 2; ++d)                              // the face from below first: the upper one's records go behind its
        if (face[d]) hipLaunchKernelGGL(k_slab_unpack2, dim3(blocks_for((size_t)msg.halo[d] + msg.mig[d])), dim3(kBlock), 0, st, face[d], d ? face[0] : (const char*)nullptr, recvCap, msg,
                                        e->d_pos[c], e->d_vel[c], e->d_rp[c], e->d_foam[c], e->d_acc, e->d_slabCnt, (uint32_t)e->cap, geom, d);
    hipLaunchKernelGGL(k_slab_commit2, dim3(1), dim3(1), 0, st, e->d_slabCnt, face[0], face[1], recvCap, (uint32_t)e->cap, msg);
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}
int sph_slab_pack_async(SphEngine* e) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) slab_hold(e);                              // an exchange outside the sized protocol (priming, re-priming after a grid change): no counts are noted for it
    e->msgSend = e->msgRecv = slab_msg_whole(e->faceCap);   // (the headers say so)
    e->intentValid = false;
    return slab_pack_on(e, e->stream);
}
int sph_slab_unpack_async(SphEngine* e, const void* recvLo, const void* recvHi, uint32_t recvCap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    return slab_unpack_on(e, e->stream, recvLo, recvHi, recvCap, slab_msg_whole(e->faceCap));
}

// ---- message sizes.  A message carries whole capacity unless the face has been CALM: the counts of the last two known exchanges (e - 3, e - 2)
// within 3 % + 64 records of each other; then it carries the count of e - 2 + a quarter + 1024.  (A face whose count grows faster than that while it
// was calm two exchanges ago gets cut off: SPH_SLAB_FLAG_TRUNCATED on the receiver, loud.  Random violent scenes showed that a margin alone is not enough:
// tools/fuzz_sweep.py, 2 of 240 slab runs with the plain "count + 25 % + 1024" rule of the first version.)
static uint32_t msg_records(uint32_t seen, uint32_t before, uint32_t cap, bool tight = false) {
    if (tight) return std::min(cap, seen);                                   // test hook (sph_slab_debug_tight_messages): no margin, no calm test
    const uint32_t hi = std::max(seen, before), lo = std::min(seen, before);
    if (hi - lo > hi / 32u + 64u) return cap;                                // not calm: the whole face
    return (uint32_t)std::min<uint64_t>(cap, (uint64_t)seen + seen / 4u + 1024u);
}
// host-only: the rule above as a function of (count two exchanges ago, count three exchanges ago, face capacity)
int sph_slab_message_records(uint32_t seen, uint32_t before, uint32_t cap) { return (int)msg_records(seen, before, cap); }

static uint32_t fnv32(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 16777619u; }
    return h;
}
constexpr uint32_t kIntentMagic = 0x504c414eu;             // "PLAN"
// THE PLAN of exchange e->exchangeNo: the records each of this engine's four messages will carry, the records it will post receives for, and the
// host-side state both derive from (exchange number, hold events, members, pause).  Everything a neighbour must agree with is in these 64 bytes:
// sph_slab_step_finish_local compares the neighbour ENGINES' plans, the RCCL transport sends the plan across each link as a fixed-size message and
// compares before a sized message is posted (slab_handshake_rccl).  The one place that reads the counts of two exchanges ago.
static int slab_plan(SphEngine* e) {
    // a member that moves the grid or the walls, noticed HERE, before the sizes (sph_slab_exchange sized its messages before anything had
    // noticed the edit; the pack that follows cuts the records for the NEW grid with a full-slot scan and may fill a face)
    {
        SphGridInfo g;
        sph::compute_grid_extents(e->params, g);
        float now[8], cont[15];
        grid_key(g, now);
        container_key(e->params, cont);
        const bool gridMoved = e->packGridValid && std::memcmp(now, e->packGrid, sizeof(now)) != 0;
        const bool wallsMoved = e->lastDt > 0.0f && std::memcmp(cont, e->lastContainer, sizeof(cont)) != 0;   // (before the first dispatch lastContainer is not a container yet)
        if (gridMoved || wallsMoved) slab_hold(e);
    }
    e->msgSend = e->msgRecv = slab_msg_whole(e->faceCap);
    const bool hold = e->calmHold > 0;                      // (host-side knowledge that every rank shares IF every rank makes the same calls: the plans' holdEvents say whether they did)
    if (hold) e->calmHold -= 1;
    if (e->exchangeNo >= 3 && !hold) {
        const int s2 = (int)((e->exchangeNo - 2u) & 3u), s3 = (int)((e->exchangeNo - 3u) & 3u);
        if (e->cntValid[s2] && e->cntValid[s3]) {
            HIP_TRY(hipEventSynchronize(e->evCnt[s2]));     // two exchanges back: long done unless the host is that far ahead of the device (the host's look-ahead is bounded by this wait)
            const SlabSeen &seen = e->h_seen[s2], &before = e->h_seen[s3];
            const bool tight = e->tightMessages != 0;
            for (int d = 0; d < 2; ++d) {
                e->msgSend.halo[d] = msg_records(seen.sent.halo[d], before.sent.halo[d], e->faceCap, tight);
                e->msgSend.mig[d] = msg_records(seen.sent.mig[d], before.sent.mig[d], e->faceCap, tight);
                e->msgRecv.halo[d] = msg_records(seen.received.halo[d], before.received.halo[d], e->faceCap, tight);
                e->msgRecv.mig[d] = msg_records(seen.received.mig[d], before.received.mig[d], e->faceCap, tight);
            }
        }
    }
    SphSlabIntent& I = e->intent;
    std::memset(&I, 0, sizeof(I));
    I.magic = kIntentMagic; I.exchangeNo = e->exchangeNo; I.stepNo = e->stepNo; I.faceCap = e->faceCap;
    for (int d = 0; d < 2; ++d) {
        const bool has = d ? e->hasHi : e->hasLo;
        e->sentBytes[d] = has ? slab_mig_msg_bytes(e->msgSend.mig[d]) + slab_halo_msg_bytes(e->msgSend.halo[d]) : 0u;
        I.sendHalo[d] = has ? e->msgSend.halo[d] : 0u; I.sendMig[d] = has ? e->msgSend.mig[d] : 0u;   // (SphSlabIntent keeps its own, public order)
        I.recvHalo[d] = has ? e->msgRecv.halo[d] : 0u; I.recvMig[d] = has ? e->msgRecv.mig[d] : 0u;
    }
    I.holdEvents = e->holdEvents;
    I.paramsHash = fnv32(&e->params, sizeof(e->params));
    I.flags = (e->params.param_pause ? 1u : 0u) | (e->tightMessages ? 2u : 0u) | (hold ? 4u : 0u);
    I.zRange = ((uint32_t)e->z0 & 0xffffu) | ((uint32_t)e->z1 << 16);
    e->intentValid = true;
    return SPH_OK;
}
// Does the plan `nb` of the neighbour on side d of `me` (0 = below, 1 = above) fit mine?  On a mismatch `why` says what differs.  Pure host logic: the
// same function judges a neighbour ENGINE's plan (one process, sph_slab_step_finish_local) and a plan received over RCCL.
static bool slab_intent_mismatch(const SphSlabIntent& me, const SphSlabIntent& nb, int d, char* why, size_t n) {
    const int o = 1 - d;                                    // the neighbour's side that faces me
    const char* side = d ? "upper" : "lower";
    if (nb.magic != kIntentMagic) { snprintf(why, n, "the %s neighbour sent no plan (magic %08x)", side, nb.magic); return true; }
    if (nb.exchangeNo != me.exchangeNo) { snprintf(why, n, "the %s neighbour is at exchange %u, this rank at %u (a rank skipped or repeated an exchange)", side, nb.exchangeNo, me.exchangeNo); return true; }
    if (nb.faceCap != me.faceCap) { snprintf(why, n, "face capacity %u here, %u on the %s neighbour", me.faceCap, nb.faceCap, side); return true; }
    const uint32_t nz0 = nb.zRange & 0xffffu, nz1 = nb.zRange >> 16, z0 = me.zRange & 0xffffu, z1 = me.zRange >> 16;
    if (d ? nz0 != z1 : nz1 != z0) { snprintf(why, n, "the %s neighbour owns layers [%u, %u), this rank [%u, %u): not adjacent", side, nz0, nz1, z0, z1); return true; }
    if (nb.holdEvents != me.holdEvents) {
        snprintf(why, n, "this rank has seen %u impulses / container edits / priming exchanges, the %s neighbour %u: one of them was issued on one rank only", me.holdEvents, side, nb.holdEvents);
        return true;
    }
    if (nb.paramsHash != me.paramsHash) { snprintf(why, n, "the members (SphParams) differ between this rank and the %s neighbour", side); return true; }
    if (nb.flags != me.flags) { snprintf(why, n, "pause / hold / message test hook differ (%u here, %u on the %s neighbour)", me.flags, nb.flags, side); return true; }
    if (nb.sendHalo[o] != me.recvHalo[d] || nb.sendMig[o] != me.recvMig[d]) {
        snprintf(why, n, "the %s neighbour will send %u halo copies + %u migrants, this rank expects %u + %u", side, nb.sendHalo[o], nb.sendMig[o], me.recvHalo[d], me.recvMig[d]);
        return true;
    }
    if (nb.recvHalo[o] != me.sendHalo[d] || nb.recvMig[o] != me.sendMig[d]) {
        snprintf(why, n, "this rank will send %u halo copies + %u migrants, the %s neighbour expects %u + %u", me.sendHalo[d], me.sendMig[d], side, nb.recvHalo[o], nb.recvMig[o]);
        return true;
    }
    return false;
}
// behind the transfer on `st`: this exchange's true counts (own: the Last* counter words; the neighbours': their headers) on their way to the host
static int slab_note_counts(SphEngine* e, hipStream_t st) {
    const int slot = (int)(e->exchangeNo & 3u);
    SlabSeen& c = e->h_seen[slot];
    HIP_TRY(hipMemcpyAsync(&c.sent, e->d_slabCnt + kSlabCntLastHaloLo, sizeof(SlabMsg), hipMemcpyDeviceToHost, st));
    for (int d = 0; d < 2; ++d) {
        c.received.halo[d] = c.received.mig[d] = 0u;
        if (d ? e->hasHi : e->hasLo) {
            HIP_TRY(hipMemcpyAsync(&c.received.halo[d], e->d_face[2 + d] + offsetof(SlabHdr, nHaloTrue), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&c.received.mig[d], e->d_face[2 + d] + offsetof(SlabHdr, nMigTrue), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipEventRecord(e->evCnt[slot], st));
    e->cntValid[slot] = true;
    e->exchangeNo += 1u;
    return SPH_OK;
}

// ---- boundary-first substep: the exchange of the next substep beside the interior of this one -------------------------
static int ensure_xstream(SphEngine* e) {
    if (e->xstream) return SPH_OK;
    {
        int least = 0, greatest = 0;                         // (numerically: greatest <= least)
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&e->xstream, hipStreamNonBlocking, greatest));   // pack / transfer / unpack: few small kernels that must not queue behind the interior's blocks
        HIP_TRY(hipStreamCreateWithPriority(&e->bstream, hipStreamNonBlocking, least));      // the interior of the SPH pass
        HIP_TRY(hipEventCreateWithFlags(&e->evSorted, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->evInterior, hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&e->evBoundary, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->evPacked, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&e->evDone));                    // (timed: sph_slab_step_times reads it as the end of the exchange)
    for (auto& ev : e->evX) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventCreate(&e->evPassEnd));
    return SPH_OK;
}
int sph_slab_step_begin(SphEngine* e, float overrideDt) {
    int rc;
    if ((rc = slab_engine(e, true))) return rc;
    if (e->stepPending) return fail(SPH_ERR_STATE, "sph_slab_step_begin twice without sph_slab_step_finish / sph_slab_step_finish_local");
    if ((rc = ensure_xstream(e))) return rc;
    if (e->params.param_pause) {                             // SPHFluid3D.cpp:432: a paused DispatchCompute is a no-op, and so is its exchange --
        e->stepPending = true; e->stepPaused = true;         // the halo records in place stay valid (impulses act on the copies as on their owners)
        e->stepNo += 1u;
        return SPH_OK;
    }
    // The halo records in place were cut by the last pack for the grid of THAT moment; a member that moves the grid (box centre / half /
    // Euler angles, h, grid_cap) must not change between two steps: the records would be classified for the old grid without a word.
    if (e->packGridValid) {
        SphGridInfo g;
        sph::compute_grid_extents(e->params, g);
        float now[8];
        grid_key(g, now);
        if (std::memcmp(now, e->packGrid, sizeof(now)) != 0)
            return fail(SPH_ERR_STATE, "the grid changed since the halo records in place were cut (box centre / half / angles, h or grid_cap edited between two steps): "
                                       "prime again with sph_slab_exchange (or pack_async / unpack_async on every engine) before the next sph_slab_step_begin");
    }
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[0], e->stream));
    e->stepNo += 1u;
    if ((rc = dispatch_one(e, overrideDt, true))) return rc;               // ... -> SPH (faces first, e->evBoundary, interior) on the engine's stream
    if ((rc = slab_plan(e))) return rc;                                      // the sizes of THIS step's exchange (the pack writes them into the headers)
    HIP_TRY(hipStreamWaitEvent(e->xstream, e->evBoundary, 0));
    for (hipEvent_t ev : e->peerDone)                                        // a neighbour engine of this process may still be copying the last send face
        if (ev) HIP_TRY(hipStreamWaitEvent(e->xstream, ev, 0));
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[1], e->xstream));
    if ((rc = slab_pack_on(e, e->xstream))) return rc;
    HIP_TRY(hipEventRecord(e->evPacked, e->xstream));
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[2], e->xstream));
    e->stepPending = true; e->stepPaused = false;
    return SPH_OK;
}
static int slab_step_join(SphEngine* e) {
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[4], e->xstream));
    HIP_TRY(hipEventRecord(e->evDone, e->xstream));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->evDone, 0));                    // the next substep's grid build sees the received records
    e->stepPending = false;
    return SPH_OK;
}
int sph_slab_step_finish_local(SphEngine* e, SphEngine* lo, SphEngine* hi) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->stepPending) return fail(SPH_ERR_STATE, "sph_slab_step_finish_local without sph_slab_step_begin");
    if ((e->hasLo != 0) != (lo != nullptr) || (e->hasHi != 0) != (hi != nullptr)) return fail(SPH_ERR_ARG, "neighbour engines do not match the slab's faces");
    for (SphEngine* nb : {lo, hi}) {
        if (!nb) continue;
        if (!nb->evPacked || nb->stepNo != e->stepNo)       // (stepNo counts the begins: the neighbour's pack of THIS step is enqueued)
            return fail(SPH_ERR_STATE, "a neighbour engine has not begun THIS step (call every engine's sph_slab_step_begin before any sph_slab_step_finish_local)");
        if (nb->stepPaused != e->stepPaused) return fail(SPH_ERR_STATE, "param_pause differs between neighbouring slab engines");
        if (nb->faceCap != e->faceCap) return fail(SPH_ERR_ARG, "face capacities differ");
    }
    if (e->stepPaused) { e->stepPending = false; return SPH_OK; }   // (stepPaused keeps saying what this step was: the neighbours compare)
    int rc;
    // Both ends of a link must have planned the same messages (each derived its sizes on its own: the sender from its counts, the receiver
    // from the headers it got, both from their own exchange number and hold state).  Here the neighbour is an engine of this process, so its
    // plan is compared directly -- what sph_slab_step_finish does with the plans it receives over RCCL.  A call issued on one engine only
    // (an impulse, a member edit, a skipped step) ends HERE, with its name, not in a truncated copy.
    if (!e->intentValid) return fail(SPH_ERR_STATE, "no plan for this exchange (sph_slab_step_begin did not run to its end)");
    for (int d = 0; d < 2; ++d) {
        SphEngine* nb = d ? hi : lo;
        if (!nb) continue;
        char why[320];
        if (!nb->intentValid || slab_intent_mismatch(e->intent, nb->intent, d, why, sizeof(why))) {
            if (!nb->intentValid) snprintf(why, sizeof(why), "the %s neighbour engine has no plan for this exchange", d ? "upper" : "lower");
            e->stepPending = false;                          // (the step cannot be finished: destroy the group or prime it again)
            return fail(SPH_ERR_STATE, "slab exchange %u refused before any record moved: %s", e->intent.exchangeNo, why);
        }
    }
    // the neighbour's send face -> this engine's receive face: header + migrants in use, halo copies in use (what sph_slab_step_finish
    // sends with ncclSend / ncclRecv), behind the neighbour's pack
    for (int d = 0; d < 2; ++d) {
        SphEngine* nb = d ? hi : lo;
        if (!nb) continue;
        const char* src = nb->d_face[d ? 0 : 1];                             // its "send lo" is my "receive hi" and the other way round
        char* dst = e->d_face[2 + d];
        HIP_TRY(hipStreamWaitEvent(e->xstream, nb->evPacked, 0));
        HIP_TRY(hipMemcpyAsync(dst, src, slab_mig_msg_bytes(e->msgRecv.mig[d]), hipMemcpyDeviceToDevice, e->xstream));
        HIP_TRY(hipMemcpyAsync(dst + slab_face_halo_off(e->faceCap), src + slab_face_halo_off(e->faceCap), slab_halo_msg_bytes(e->msgRecv.halo[d]), hipMemcpyDeviceToDevice, e->xstream));
    }
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[3], e->xstream));
    if ((rc = slab_unpack_on(e, e->xstream, e->d_face[2], e->d_face[3], e->faceCap, e->msgRecv))) return rc;
    if ((rc = slab_note_counts(e, e->xstream))) return rc;
    if ((rc = slab_step_join(e))) return rc;
    if (lo) lo->peerDone[1] = e->evDone;                                     // their next pack overwrites the face this engine has just read
    if (hi) hi->peerDone[0] = e->evDone;
    return SPH_OK;
}
int sph_slab_status(SphEngine* e, uint32_t out[5]) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (int rc = slab_engine(e)) return rc;
    uint32_t host[kSlabCntPackedHi + 1];
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->xstream) HIP_TRY(hipStreamSynchronize(e->xstream));
    HIP_TRY(hipMemcpyAsync(host, e->d_slabCnt, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i <= kSlabCntFlags; ++i) out[i] = host[i];   // out[5] is the first five counter words ...
    out[0] += host[kSlabCntPackedLo]; out[1] += host[kSlabCntPackedHi];   // ... plus the async pack's counts (the header kernel resets the running ones)
    return slab_flags_error(e, host[kSlabCntFlags], out[0], out[1]);    // (SPH_SLAB_FLAG_LAYER_JUMP alone is a notice, not an error: out[4] carries it)
}
int sph_slab_clear_flags(SphEngine* e, uint32_t mask) {
    if (int rc = slab_engine(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->xstream) HIP_TRY(hipStreamSynchronize(e->xstream));
    uint32_t f = 0;
    HIP_TRY(hipMemcpy(&f, e->d_slabCnt + kSlabCntFlags, sizeof(f), hipMemcpyDeviceToHost));
    f &= ~mask;
    HIP_TRY(hipMemcpy(e->d_slabCnt + kSlabCntFlags, &f, sizeof(f), hipMemcpyHostToDevice));
    return SPH_OK;
}
int sph_slab_message_bytes(SphEngine* e, uint64_t out[4]) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->slab || !e->faceCap) return fail(SPH_ERR_STATE, "slab engine with face buffers required");
    out[0] = e->sentBytes[0]; out[1] = e->sentBytes[1];
    out[2] = e->hasLo ? (uint64_t)slab_face_bytes(e->faceCap) : 0u; out[3] = e->hasHi ? (uint64_t)slab_face_bytes(e->faceCap) : 0u;
    return SPH_OK;
}
int sph_slab_step_times(SphEngine* e, float outMs[5]) {
    if (!e || !outMs) return fail(SPH_ERR_ARG, "null argument");
    if (!e->slab || !e->xstream || !e->optTiming) return fail(SPH_ERR_STATE, "needs a slab engine that has run a boundary-first step with SPH_OPT_TIMING on");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->xstream));
    // {pack, transfer, unpack} durations on the exchange stream, then when the exchange ended and when the SPH pass ended, both measured from the pass's start
    float v[5] = {0, 0, 0, 0, 0};
    hipError_t er = hipEventElapsedTime(&v[0], e->evX[1], e->evX[2]);
    if (er == hipSuccess) er = hipEventElapsedTime(&v[1], e->evX[2], e->evX[3]);
    if (er == hipSuccess) er = hipEventElapsedTime(&v[2], e->evX[3], e->evX[4]);
    if (er == hipSuccess) er = hipEventElapsedTime(&v[3], e->evX[0], e->evX[4]);
    if (er == hipSuccess && e->evPassEnd) er = hipEventElapsedTime(&v[4], e->evX[0], e->evPassEnd);
    if (er != hipSuccess) return fail(SPH_ERR_STATE, "no timed boundary-first step yet: %s", hipGetErrorString(er));
    for (int i = 0; i < 5; ++i) outMs[i] = v[i];
    return SPH_OK;
}

}  // extern "C"

// RCCL is loaded at run time (dlopen): the library has no link-time dependency on it, and a host without RCCL still loads
// the engine (the exchange then fails with a message).
#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.lib) return SPH_OK;
    void* h = nullptr;
    // SPH_RCCL_LIBRARY names the library that provides the nccl* entry points (default: librccl.so.1).  The tests put a stand-in there that moves the messages
    // between PROCESSES ON ONE GPU through shared memory and REFUSES a receive whose size differs from its send's (tests/fake_rccl/): the engine's own multi-rank
    // code -- plans, grouped face messages, unpack -- then runs between real ranks on a one-GPU box, where RCCL itself refuses two ranks on one device.
    if (const char* over = std::getenv("SPH_RCCL_LIBRARY")) {
        h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(SPH_ERR_HIP, "SPH_RCCL_LIBRARY=%s cannot be loaded: %s", over, dlerror());
    }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { if (h) break; h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); }
    if (!h) return fail(SPH_ERR_HIP, "RCCL not available: %s", dlerror());
    Rccl r;
    r.lib = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.Send = (decltype(r.Send))dlsym(h, "ncclSend");
    r.Recv = (decltype(r.Recv))dlsym(h, "ncclRecv");
    r.AllReduce = (decltype(r.AllReduce))dlsym(h, "ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.Send || !r.Recv || !r.AllReduce || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
        dlclose(h);
        return fail(SPH_ERR_HIP, "RCCL library lacks a required entry point");
    }
    g_rccl = r;
    return SPH_OK;
}
#define NCCL_TRY(expr)                                                                                         \
    do {                                                                                                       \
        ncclResult_t _r = (expr);                                                                              \
        if (_r != ncclSuccess) return fail(SPH_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(_r));   \
    } while (0)
}  // namespace

struct SphComm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
};

extern "C" {

int sph_comm_unique_id(void* out128) {
    if (!out128) return fail(SPH_ERR_ARG, "null argument");
    static_assert(sizeof(ncclUniqueId) == SPH_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    int rc;
    if ((rc = rccl_load())) return rc;
    ncclUniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    std::memcpy(out128, &id, sizeof(id));
    return SPH_OK;
}
int sph_comm_create(SphComm** out, const void* id128, int rank, int world) {
    if (!out || !id128) return fail(SPH_ERR_ARG, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(SPH_ERR_ARG, "bad rank %d of %d", rank, world);
    int rc;
    if ((rc = rccl_load())) return rc;
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    SphComm* c = new SphComm();
    c->rank = rank; c->world = world;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, id, rank);       // one rank per process, on the current HIP device
    if (r != ncclSuccess) { delete c; return fail(SPH_ERR_HIP, "ncclCommInitRank failed: %s", g_rccl.GetErrorString(r)); }
    *out = c;
    return SPH_OK;
}
int sph_comm_destroy(SphComm* c) {
    if (!c) return SPH_OK;
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    delete c;
    return SPH_OK;
}
// Health check of the transport on THIS rank alone: one grouped ncclSend + ncclRecv of `bytes` bytes from the rank to
// itself (RCCL serves a self send / recv with a device copy), issued the way slab_transfer_rccl issues the face messages
// (ncclUint8 counts, a non-blocking stream that is not the null stream), then compared word for word on the host.
// It is the only way to run ncclSend / ncclRecv on a box with one GPU (RCCL refuses two ranks on one device).
int sph_comm_selftest(SphComm* c, uint64_t bytes) { return sph_comm_selftest_timed(c, bytes, nullptr); }
// (msOut: hipEvent time of the grouped send + receive alone)
int sph_comm_selftest_timed(SphComm* c, uint64_t bytes, float* msOut) {
    if (!c || !c->comm) return fail(SPH_ERR_ARG, "null communicator");
    if (bytes == 0 || bytes > (1ull << 30) || (bytes & 3ull)) return fail(SPH_ERR_ARG, "bytes must be a multiple of 4 in (0, 2^30]");
    const size_t words = (size_t)(bytes / 4);
    uint32_t *src = nullptr, *dst = nullptr;
    hipStream_t st = nullptr;
    int rc = SPH_OK;
    std::vector<uint32_t> host(words);
    auto cleanup = [&]() { if (st) (void)hipStreamDestroy(st); if (src) (void)hipFree(src); if (dst) (void)hipFree(dst); };
    if ((rc = dev_alloc(&src, words)) || (rc = dev_alloc(&dst, words))) { cleanup(); return rc; }
    hipError_t er = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (size_t i = 0; i < words; ++i) host[i] = (uint32_t)i * 2654435761u + 12345u;
    if (er == hipSuccess) er = hipMemcpyAsync(src, host.data(), bytes, hipMemcpyHostToDevice, st);
    if (er == hipSuccess) er = hipMemsetAsync(dst, 0, bytes, st);
    if (er != hipSuccess) { cleanup(); return fail(SPH_ERR_HIP, "self-test setup failed: %s", hipGetErrorString(er)); }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (msOut) { (void)hipEventCreate(&t0); (void)hipEventCreate(&t1); (void)hipEventRecord(t0, st); }
    ncclResult_t g0 = g_rccl.GroupStart();
    ncclResult_t r = g0;
    if (r == ncclSuccess) r = g_rccl.Send(src, (size_t)bytes, ncclUint8, c->rank, c->comm, st);
    if (r == ncclSuccess) r = g_rccl.Recv(dst, (size_t)bytes, ncclUint8, c->rank, c->comm, st);
    ncclResult_t g1 = g0 == ncclSuccess ? g_rccl.GroupEnd() : g0;
    if (msOut) {
        *msOut = 0.0f;
        (void)hipEventRecord(t1, st);
        if (hipEventSynchronize(t1) == hipSuccess) (void)hipEventElapsedTime(msOut, t0, t1);
        (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    }
    if (r != ncclSuccess || g1 != ncclSuccess) {
        (void)hipStreamSynchronize(st);
        cleanup();
        return fail(SPH_ERR_HIP, "self send / recv failed: %s", g_rccl.GetErrorString(r != ncclSuccess ? r : g1));
    }
    std::vector<uint32_t> back(words);
    er = hipMemcpyAsync(back.data(), dst, bytes, hipMemcpyDeviceToHost, st);
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    cleanup();
    if (er != hipSuccess) return fail(SPH_ERR_HIP, "self-test copy back failed: %s", hipGetErrorString(er));
    for (size_t i = 0; i < words; ++i)
        if (back[i] != host[i]) return fail(SPH_ERR_HIP, "self send / recv delivered wrong data at word %zu of %zu", i, words);
    return SPH_OK;
}
// What every call that takes a communicator checks first: the engine's neighbours are the communicator's, and all ranks allocated the same faces.
static int slab_check_comm(SphEngine* e, SphComm* c) {
    if (!e || !c) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = slab_engine(e, true))) return rc;
    // both directions: a rank that waits for a neighbour the neighbour does not know about would hang in ncclRecv
    if ((e->hasLo != 0) != (c->rank > 0) || (e->hasHi != 0) != (c->rank < c->world - 1))
        return fail(SPH_ERR_ARG, "slab neighbours (lo %d, hi %d) do not match rank %d of %d", e->hasLo, e->hasHi, c->rank, c->world);
    if (e->faceAgreedWith != c) {
        // Once per (engine, communicator): the face capacity is the size of every message, so all ranks must have
        // allocated the same one -- a mismatch would otherwise show up as a hang inside ncclSend / ncclRecv.
        uint32_t* d = nullptr;
        if ((rc = dev_alloc(&d, 2))) return rc;
        const uint32_t mine[2] = {e->faceCap, ~e->faceCap};
        uint32_t agreed[2] = {0, 0};
        hipError_t er = hipMemcpyAsync(d, mine, sizeof(mine), hipMemcpyHostToDevice, e->stream);
        ncclResult_t nr = ncclSuccess;
        if (er == hipSuccess) nr = g_rccl.AllReduce(d, d, 2, ncclUint32, ncclMax, c->comm, e->stream);
        if (er == hipSuccess && nr == ncclSuccess) er = hipMemcpyAsync(agreed, d, sizeof(agreed), hipMemcpyDeviceToHost, e->stream);
        if (er == hipSuccess && nr == ncclSuccess) er = hipStreamSynchronize(e->stream);
        (void)hipFree(d);
        if (nr != ncclSuccess) return fail(SPH_ERR_HIP, "ncclAllReduce failed: %s", g_rccl.GetErrorString(nr));
        if (er != hipSuccess) return fail(SPH_ERR_HIP, "face capacity agreement failed: %s", hipGetErrorString(er));
        if (agreed[0] != e->faceCap || agreed[1] != ~e->faceCap)
            return fail(SPH_ERR_ARG, "face capacity %u differs between ranks (largest %u, smallest %u): sph_slab_alloc_faces must be given the same value everywhere",
                        e->faceCap, agreed[0], ~agreed[1]);
        e->faceAgreedWith = c;
    }
    return SPH_OK;
}
// The grouped ncclSend / ncclRecv of one exchange's faces: per neighbour TWO send / receive pairs in ONE group -- header + the migrants in use, and the
// halo copies in use -- of unequal sizes.  One routine for the engine's exchange (slab_transfer_rccl) and for the self-test that runs exactly this
// pattern on a one-GPU box with the rank itself as both neighbours (sph_comm_selftest_faces): ncclSend / ncclRecv to one peer match in issue order.
static int rccl_post_faces(SphComm* c, hipStream_t st, const int peer[2], const bool has[2], char* const sendFace[2], char* const recvFace[2],
                           const SlabMsg& msgSend, const SlabMsg& msgRecv, uint32_t faceCap) {
    if (!has[0] && !has[1]) return SPH_OK;
    const size_t hoff = slab_face_halo_off(faceCap);
    NCCL_TRY(g_rccl.GroupStart());
    ncclResult_t r = ncclSuccess;
    for (int d = 0; d < 2 && r == ncclSuccess; ++d) {
        if (!has[d]) continue;
        r = g_rccl.Send(sendFace[d], slab_mig_msg_bytes(msgSend.mig[d]), ncclUint8, peer[d], c->comm, st);
        if (r == ncclSuccess) r = g_rccl.Send(sendFace[d] + hoff, slab_halo_msg_bytes(msgSend.halo[d]), ncclUint8, peer[d], c->comm, st);
        if (r == ncclSuccess) r = g_rccl.Recv(recvFace[d], slab_mig_msg_bytes(msgRecv.mig[d]), ncclUint8, peer[d], c->comm, st);
        if (r == ncclSuccess) r = g_rccl.Recv(recvFace[d] + hoff, slab_halo_msg_bytes(msgRecv.halo[d]), ncclUint8, peer[d], c->comm, st);
    }
    ncclResult_t g = g_rccl.GroupEnd();
    if (r != ncclSuccess) return fail(SPH_ERR_HIP, "ncclSend / ncclRecv failed: %s", g_rccl.GetErrorString(r));
    if (g != ncclSuccess) return fail(SPH_ERR_HIP, "ncclGroupEnd failed: %s", g_rccl.GetErrorString(g));
    return SPH_OK;
}
static int slab_transfer_rccl(SphEngine* e, SphComm* c, hipStream_t st) {
    const int peer[2] = {c->rank - 1, c->rank + 1};
    const bool has[2] = {e->hasLo != 0, e->hasHi != 0};
    return rccl_post_faces(c, st, peer, has, e->d_face, e->d_face + 2, e->msgSend, e->msgRecv, e->faceCap);   // send lo / hi, receive lo / hi
}
// A wait for a neighbour that cannot hang the host: the event is polled, and after `seconds` the call fails (SPH_ERR_TIMEOUT).  The work behind the
// event is then still queued on the device (a receive whose sender never came): the process has to end; nothing can be re-posted on this communicator.
static int wait_event_deadline(hipEvent_t ev, double seconds, float* waitedMs) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(ev);
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waitedMs) *waitedMs = (float)(el * 1e3);
        if (q == hipSuccess) return SPH_OK;
        if (q != hipErrorNotReady) return fail(SPH_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        if (el > seconds) return SPH_ERR_TIMEOUT;
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50)); else std::this_thread::yield();
    }
}
// The fixed-size message that precedes the sized ones: every rank sends its PLAN (64 bytes, slab_plan) to its neighbours and receives theirs.  Its size
// depends on nothing, so it cannot be mismatched.
static int rccl_post_plans(SphComm* c, hipStream_t st, const int peer[2], const bool has[2], SlabPlans* d_plans) {
    if (!has[0] && !has[1]) return SPH_OK;
    NCCL_TRY(g_rccl.GroupStart());
    ncclResult_t r = ncclSuccess;
    for (int d = 0; d < 2 && r == ncclSuccess; ++d) {
        if (!has[d]) continue;
        r = g_rccl.Send(&d_plans->mine, sizeof(SphSlabIntent), ncclUint8, peer[d], c->comm, st);
        if (r == ncclSuccess) r = g_rccl.Recv(&d_plans->from[d], sizeof(SphSlabIntent), ncclUint8, peer[d], c->comm, st);
    }
    ncclResult_t g = g_rccl.GroupEnd();
    if (r != ncclSuccess) return fail(SPH_ERR_HIP, "ncclSend / ncclRecv of the plans failed: %s", g_rccl.GetErrorString(r));
    if (g != ncclSuccess) return fail(SPH_ERR_HIP, "ncclGroupEnd failed: %s", g_rccl.GetErrorString(g));
    return SPH_OK;
}
static int ensure_handshake(SphEngine* e) {
    if (e->hstream) return SPH_OK;
    int rc;
    if ((rc = dev_alloc(&e->d_intent, 1))) return rc;
    HIP_TRY(hipHostMalloc((void**)&e->h_intent, sizeof(SlabPlans), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&e->evIntent, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&e->hstream, hipStreamNonBlocking));
    return SPH_OK;
}
// BEFORE a sized message of this exchange is posted: the plans cross each link and are compared on the host (SPH_SLAB_VERIFY 1, the default).  What this
// costs: one more grouped send / receive of 64 bytes per neighbour on a stream of its own, and a host wait until the neighbours have reached the same
// exchange -- which bounds the host's look-ahead to about one exchange (the device still holds more than a substep of queued work meanwhile).  What it
// buys: two ranks whose host-side state went apart (an impulse, a member edit, an upload or a skipped step on one rank only) get an error with the
// difference by name on BOTH ranks, where the sized ncclSend / ncclRecv would have hung or cut records off; and a neighbour that never arrives is a
// timeout with this rank's step and sizes, not a hang.
static int slab_handshake_rccl(SphEngine* e, SphComm* c) {
    if (!e->verifyMode || !(e->hasLo || e->hasHi)) return SPH_OK;
    if (!e->intentValid) return fail(SPH_ERR_STATE, "no plan for this exchange");
    int rc;
    if ((rc = ensure_handshake(e))) return rc;
    e->h_intent->mine = e->intent;
    std::memset(e->h_intent->from, 0, sizeof(e->h_intent->from));
    HIP_TRY(hipMemcpyAsync(e->d_intent, e->h_intent, sizeof(SlabPlans), hipMemcpyHostToDevice, e->hstream));
    const int peer[2] = {c->rank - 1, c->rank + 1};
    const bool has[2] = {e->hasLo != 0, e->hasHi != 0};
    if ((rc = rccl_post_plans(c, e->hstream, peer, has, e->d_intent))) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_intent->from, e->d_intent->from, sizeof(e->h_intent->from), hipMemcpyDeviceToHost, e->hstream));
    HIP_TRY(hipEventRecord(e->evIntent, e->hstream));
    rc = wait_event_deadline(e->evIntent, e->deadlineSec, &e->handshakeMs);
    e->handshakes += 1u;
    if (rc == SPH_ERR_TIMEOUT)
        return fail(SPH_ERR_TIMEOUT, "rank %d of %d: no plan from a neighbour within %.1f s at exchange %u (step %u; this rank would send %u + %u records down, %u + %u up): "
                                     "a neighbour rank is not making the same calls, or is gone.  The receive stays queued on the device: end this process.",
                    c->rank, c->world, e->deadlineSec, e->intent.exchangeNo, e->stepNo, e->intent.sendHalo[0], e->intent.sendMig[0], e->intent.sendHalo[1], e->intent.sendMig[1]);
    if (rc) return rc;
    for (int d = 0; d < 2; ++d) {
        if (!has[d]) continue;
        char why[320];
        if (slab_intent_mismatch(e->intent, e->h_intent->from[d], d, why, sizeof(why)))
            return fail(SPH_ERR_STATE, "rank %d of %d: slab exchange %u refused before any record moved: %s", c->rank, c->world, e->intent.exchangeNo, why);
    }
    return SPH_OK;
}
// One halo exchange of a substep: plan -> (the plans cross the links and are compared) -> pack -> per z-neighbour two grouped ncclSend / ncclRecv pairs -> unpack,
// enqueued on the engine's stream; the stream order makes the unpack wait for the receives and the next pack wait for the sends.  With SPH_SLAB_VERIFY 0
// there is no host wait on the path at all (the sizes come from counts that are two exchanges old).
int sph_slab_exchange(SphEngine* e, SphComm* c) {
    int rc;
    if ((rc = slab_check_comm(e, c))) return rc;
    if (e->stepPending) return fail(SPH_ERR_STATE, "a boundary-first step is pending: finish it with sph_slab_step_finish");
    if (e->params.param_pause) return SPH_OK;                // the paused sph_dispatch that follows is a no-op: the halo records in place stay valid
    if ((rc = slab_plan(e))) return rc;
    if ((rc = slab_handshake_rccl(e, c))) return rc;
    if ((rc = slab_pack_on(e, e->stream))) return rc;
    if ((rc = slab_transfer_rccl(e, c, e->stream))) return rc;
    if ((rc = slab_unpack_on(e, e->stream, e->d_face[2], e->d_face[3], e->faceCap, e->msgRecv))) return rc;
    return slab_note_counts(e, e->stream);
}
// Second half of a boundary-first substep with RCCL as the transport: the transfer and the unpack follow the pack on the
// exchange stream; the engine's stream (the interior of the SPH pass) only waits for them at its end.
int sph_slab_step_finish(SphEngine* e, SphComm* c) {
    int rc;
    if ((rc = slab_check_comm(e, c))) return rc;
    if (!e->stepPending) return fail(SPH_ERR_STATE, "sph_slab_step_finish without sph_slab_step_begin");
    if (e->stepPaused) { e->stepPending = false; return SPH_OK; }
    if ((rc = slab_handshake_rccl(e, c))) { e->stepPending = false; return rc; }   // (the plan is sph_slab_step_begin's)
    if ((rc = slab_transfer_rccl(e, c, e->xstream))) return rc;
    if (e->optTiming) HIP_TRY(hipEventRecord(e->evX[3], e->xstream));
    if ((rc = slab_unpack_on(e, e->xstream, e->d_face[2], e->d_face[3], e->faceCap, e->msgRecv))) return rc;
    if ((rc = slab_note_counts(e, e->xstream))) return rc;
    return slab_step_join(e);
}

// ---- the agreement protocol's knobs and its view from outside ----
int sph_slab_set_verify(SphEngine* e, int mode) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (mode < 0 || mode > 1) return fail(SPH_ERR_ARG, "verify mode %d: 1 = the plans cross the links before every sized exchange (default), 0 = off", mode);
    e->verifyMode = mode;
    return SPH_OK;
}
int sph_slab_set_deadline(SphEngine* e, double seconds) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!(seconds > 0.0)) return fail(SPH_ERR_ARG, "deadline must be > 0 s");
    e->deadlineSec = seconds;
    return SPH_OK;
}
int sph_slab_plan(const SphEngine* e, SphSlabIntent* out, float* handshakeMsOut) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (int rc = slab_engine(e)) return rc;
    if (!e->intentValid) return fail(SPH_ERR_STATE, "no sized exchange has been planned yet");
    *out = e->intent;
    if (handshakeMsOut) *handshakeMsOut = e->handshakeMs;
    return SPH_OK;
}
int sph_slab_plans_agree(const SphSlabIntent* mine, const SphSlabIntent* neighbour, int side, char* why, size_t whyBytes) {
    if (!mine || !neighbour || side < 0 || side > 1) return fail(SPH_ERR_ARG, "bad argument");
    char buf[320];
    buf[0] = 0;
    const bool bad = slab_intent_mismatch(*mine, *neighbour, side, buf, sizeof(buf));
    if (why && whyBytes) { std::strncpy(why, buf, whyBytes - 1); why[whyBytes - 1] = 0; }
    return bad ? 0 : 1;
}
int sph_slab_debug_tight_messages(SphEngine* e, int on) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    e->tightMessages = on ? 1 : 0;
    return SPH_OK;
}
// Exactly the engine's exchange pattern over RCCL on ONE rank (the rank is its own lower and upper neighbour): the 64-byte plans first (with the
// polled, deadline-bounded wait of the handshake), then rccl_post_faces -- the routine slab_transfer_rccl calls -- with two send / receive pairs of
// UNEQUAL sizes per neighbour in one group, and every byte compared afterwards: what arrived is what was sent, nothing beyond a message was touched.
int sph_comm_selftest_faces(SphComm* c, uint32_t faceCap, const uint32_t counts[4] /* halo lo, halo hi, migrants lo, migrants hi */, float* msOut) {
    if (!c || !c->comm || !counts) return fail(SPH_ERR_ARG, "null argument");
    if (faceCap == 0 || faceCap > (1u << 24)) return fail(SPH_ERR_ARG, "face capacity %u out of range", faceCap);
    for (int i = 0; i < 4; ++i) if (counts[i] > faceCap) return fail(SPH_ERR_ARG, "count %u > face capacity %u", counts[i], faceCap);
    const size_t fb = slab_face_bytes(faceCap), hoff = slab_face_halo_off(faceCap);
    char* face[4] = {nullptr, nullptr, nullptr, nullptr};
    SlabPlans* d_plans = nullptr;
    hipStream_t st = nullptr, hs = nullptr;
    hipEvent_t ev = nullptr, t0 = nullptr, t1 = nullptr;
    auto cleanup = [&]() {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        if (hs) { (void)hipStreamSynchronize(hs); (void)hipStreamDestroy(hs); }
        for (auto& f : face) if (f) (void)hipFree(f);
        if (d_plans) (void)hipFree(d_plans);
        for (hipEvent_t x : {ev, t0, t1}) if (x) (void)hipEventDestroy(x);
    };
    int rc = SPH_OK;
    for (int i = 0; i < 4 && !rc; ++i) rc = dev_alloc(&face[i], fb);
    if (!rc) rc = dev_alloc(&d_plans, 1);
    if (rc) { cleanup(); return rc; }
    hipError_t er = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (er == hipSuccess) er = hipStreamCreateWithFlags(&hs, hipStreamNonBlocking);
    if (er == hipSuccess) er = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (er == hipSuccess) er = hipEventCreate(&t0);
    if (er == hipSuccess) er = hipEventCreate(&t1);
    std::vector<unsigned char> host[2];
    for (int d = 0; d < 2 && er == hipSuccess; ++d) {
        host[d].resize(fb);
        for (size_t i = 0; i < fb; ++i) host[d][i] = (unsigned char)((i * 2654435761u + 977u * (unsigned)d + (i >> 11)) >> 7);
        er = hipMemcpyAsync(face[d], host[d].data(), fb, hipMemcpyHostToDevice, st);
        if (er == hipSuccess) er = hipMemsetAsync(face[2 + d], 0, fb, st);
    }
    if (er == hipSuccess) er = hipStreamSynchronize(st);
    if (er != hipSuccess) { cleanup(); return fail(SPH_ERR_HIP, "self-test setup failed: %s", hipGetErrorString(er)); }
    const int peer[2] = {c->rank, c->rank};
    const bool has[2] = {true, true};
    // the plans
    constexpr int planWords = (int)(sizeof(SphSlabIntent) / sizeof(uint32_t));
    uint32_t pattern[planWords];
    for (int i = 0; i < planWords; ++i) pattern[i] = 0x504c0000u + (uint32_t)i;
    SlabPlans plans{}, back;
    std::memcpy(&plans.mine, pattern, sizeof(pattern));
    er = hipMemcpyAsync(d_plans, &plans, sizeof(plans), hipMemcpyHostToDevice, hs);
    if (er == hipSuccess) er = hipStreamSynchronize(hs);
    if (er != hipSuccess) { cleanup(); return fail(SPH_ERR_HIP, "self-test setup failed: %s", hipGetErrorString(er)); }
    if ((rc = rccl_post_plans(c, hs, peer, has, d_plans))) { cleanup(); return rc; }
    (void)hipEventRecord(ev, hs);
    float waited = 0.0f;
    rc = wait_event_deadline(ev, 20.0, &waited);
    if (rc) { cleanup(); return rc == SPH_ERR_TIMEOUT ? fail(SPH_ERR_TIMEOUT, "the plans' send / receive to self did not complete within 20 s") : rc; }
    er = hipMemcpy(&back, d_plans, sizeof(back), hipMemcpyDeviceToHost);
    if (er != hipSuccess) { cleanup(); return fail(SPH_ERR_HIP, "self-test copy back failed: %s", hipGetErrorString(er)); }
    uint32_t words[2 * planWords];
    std::memcpy(words, back.from, sizeof(words));
    for (int i = 0; i < 2 * planWords; ++i)
        if (words[i] != pattern[i % planWords]) { cleanup(); return fail(SPH_ERR_HIP, "a 64-byte plan sent to self arrived wrong at word %d", i); }
    // the faces: the sizes a receiver posts are the sizes the matching sender uses (what the plans' comparison guarantees between two ranks)
    (void)hipEventRecord(t0, st);
    const SlabMsg msg{{counts[0], counts[1]}, {counts[2], counts[3]}};   // (the public order: halo lo, halo hi, migrants lo, migrants hi)
    if ((rc = rccl_post_faces(c, st, peer, has, face, face + 2, msg, msg, faceCap))) { cleanup(); return rc; }
    (void)hipEventRecord(t1, st);
    rc = wait_event_deadline(t1, 60.0, nullptr);
    if (rc) { cleanup(); return rc == SPH_ERR_TIMEOUT ? fail(SPH_ERR_TIMEOUT, "the face messages to self did not complete within 60 s") : rc; }
    if (msOut) { *msOut = 0.0f; (void)hipEventElapsedTime(msOut, t0, t1); }
    std::vector<unsigned char> got(fb);
    for (int d = 0; d < 2; ++d) {
        er = hipMemcpy(got.data(), face[2 + d], fb, hipMemcpyDeviceToHost);
        if (er != hipSuccess) { cleanup(); return fail(SPH_ERR_HIP, "self-test copy back failed: %s", hipGetErrorString(er)); }
        const size_t migEnd = slab_mig_msg_bytes(msg.mig[d]), haloEnd = hoff + slab_halo_msg_bytes(msg.halo[d]);
        for (size_t i = 0; i < fb; ++i) {
            const bool sent = i < migEnd || (i >= hoff && i < haloEnd);
            const unsigned char want = sent ? host[d][i] : (unsigned char)0;
            if (got[i] != want) { cleanup(); return fail(SPH_ERR_HIP, "face %d: byte %zu of %zu is %u, expected %u (%s a message)", d, i, fb, got[i], want, sent ? "inside" : "beyond"); }
        }
    }
    cleanup();
    return SPH_OK;
}

int sph_sync(SphEngine* e) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->xstream) HIP_TRY(hipStreamSynchronize(e->xstream));
    return SPH_OK;
}
// sph_sync that cannot hang: the engine's streams are polled, and after `seconds` (<= 0: the engine's deadline, sph_slab_set_deadline) the call fails with
// SPH_ERR_TIMEOUT and says where this engine stands.  For multi-rank hosts (bench.py --gpus N, halo.SlabSimulation): a transfer whose peer never posted
// its half keeps the stream busy for ever; the host prints the message and ends the process (a fresh process, never a re-exec).
int sph_sync_deadline(SphEngine* e, double seconds) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    const double limit = seconds > 0.0 ? seconds : e->deadlineSec;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t sts[4] = {e->stream, e->xstream, e->bstream, e->hstream};
    for (unsigned spins = 0;; ++spins) {
        bool busy = false;
        for (hipStream_t st : sts) {
            if (!st) continue;
            const hipError_t q = hipStreamQuery(st);
            if (q == hipErrorNotReady) busy = true;
            else if (q != hipSuccess) return fail(SPH_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        }
        if (!busy) return SPH_OK;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > limit)
            return fail(SPH_ERR_TIMEOUT, "the engine's streams did not drain within %.1f s (boundary-first steps begun %u, sized exchanges enqueued %u, last plan: %u + %u records down, %u + %u up): "
                                         "a transfer is waiting for a neighbour rank that never posted its half.  End this process.",
                        limit, e->stepNo, e->exchangeNo, e->intent.sendHalo[0], e->intent.sendMig[0], e->intent.sendHalo[1], e->intent.sendMig[1]);
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(100)); else std::this_thread::yield();
    }
}

// ---- field sampling (sph_sample.h) ---------------------------------------------------------------
// What no query of the current state supports: a z-slab engine, the linked-list grid.  Entry points that allocate state this first.
static int query_refused(const SphEngine* e) {
    if (e->slab) return fail(SPH_ERR_STATE, "sampling a z-slab engine is not supported: its halo records after a step are the step's entry state");
    return needs_sorted_copy(e, "sampling needs");
}
// The grid of the CURRENT state, built outside a substep exactly as sph_download_grid builds it.  The next dispatch builds its
// own (dispatch_one always does), so nothing of this build reaches the simulation.
static int sample_grid(SphEngine* e, SimK& k, bool orderAll = false) {
    int rc;
    if ((rc = query_refused(e)) || (rc = validate_params(e->params))) return rc;
    sph::compute_grid_extents(e->params, e->grid);
    if ((rc = ensure_grid_buffers(e))) return rc;
    make_simk(e->params, e->grid, e->params.param_timeStep, k);
    if ((rc = import_state(e))) return rc;
    return build_grid(e, k, false, orderAll);
}

// How every query that checks arguments against the grid opens: the refusal, then the params, then the grid they give (for the cell
// size and the cell count).  Nothing is allocated and nothing of the engine changes; the caller's order from here on is argument
// check, allocation, sample_grid.
static int query_grid(const SphEngine* e, SphGridInfo& g) {
    int rc;
    if ((rc = query_refused(e)) || (rc = validate_params(e->params))) return rc;
    sph::compute_grid_extents(e->params, g);
    return SPH_OK;
}

// A search radius as an argument: the stencil half-width through *stencil.
static int radius_stencil(float radius, float cellSize, int* stencil) {
    *stencil = sph::neighbor_stencil(radius, cellSize);
    if (!*stencil) return fail(SPH_ERR_ARG, "radius %g is not finite, not > 0 or above three cells (%g)", (double)radius, (double)(3.0f * cellSize));
    return SPH_OK;
}
// ids[slot] of the grid sample_grid has just built, into d_slotIds (grown by the caller).
static void slot_ids_fill(SphEngine* e) {
    if (!e->n) return;
    Timed t(e, SPH_K_OTHER);
    hipLaunchKernelGGL(k_neighbors_ids, dim3(blocks_for(e->n)), dim3(kBlock), 0, e->stream, (const float4*)e->d_sOwn, e->d_slotIds.p, e->idBase, (uint32_t)e->n);
}
// The 64-bit exclusive scan of cnt[0 .. rows) into offsets[0 .. rows], rows > 0, on the queries' scratch (scanScratch.grow first): the
// three launches in one bracket.  One synchronisation: hostTotals[0 .. 2).
static int scan_counts64(SphEngine* e, const uint32_t* cnt, size_t rows, long long* offsets, unsigned long long hostTotals[2]) {
    unsigned long long* totals;
    {
        Timed t(e, SPH_K_OTHER);
        totals = scan_counts64_launch(e, e->scanScratch, cnt, rows, offsets);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hostTotals, totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// A regular lattice of points as an argument: at least `least` points along every axis, a finite spacing > 0, at most 2^31 - 1 points.
static int check_lattice(const int dims[3], const float spacing[3], int least, long long* totalOut) {
    if (!dims || !spacing) return fail(SPH_ERR_ARG, "null argument");
    long long total = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < least) return fail(SPH_ERR_ARG, "lattice dimension %d is %d (must be >= %d)", a, dims[a], least);
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0f)) return fail(SPH_ERR_ARG, "lattice spacing %d is %g (must be finite and > 0)", a, (double)spacing[a]);
        total *= dims[a];
        if (total > 2147483647ll) return fail(SPH_ERR_ARG, "lattice of %d x %d x %d points exceeds 2^31 - 1 points", dims[0], dims[1], dims[2]);
    }
    if (totalOut) *totalOut = total;
    return SPH_OK;
}

// The constants of a lattice kernel (arguments already checked): the 8 x 8 x 4 bricks of k_sample_lattice and k_aniso_lattice.
static sph::LatticeK lattice_consts(const float origin[3], const float spacing[3], const int dims[3], int field, int stage) {
    using namespace sph;
    LatticeK L;
    L.ox = origin[0]; L.oy = origin[1]; L.oz = origin[2];
    L.sx = spacing[0]; L.sy = spacing[1]; L.sz = spacing[2];
    L.dx = dims[0]; L.dy = dims[1]; L.dz = dims[2];
    L.nbx = (dims[0] + kBrickX - 1) / kBrickX; L.nby = (dims[1] + kBrickY - 1) / kBrickY;
    L.nBricks = (long long)L.nbx * L.nby * ((dims[2] + kBrickZ - 1) / kBrickZ);
    L.field = field;
    L.stage = stage;
    return L;
}

int sph_sample_points_device(SphEngine* e, const float* devPoints4, size_t m, SphSample* devOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (m && (!devPoints4 || !devOut)) return fail(SPH_ERR_ARG, "null argument");
    if (m > (size_t)1 << 40) return fail(SPH_ERR_ARG, "%zu probes", m);
    SimK k;
    int rc;
    if ((rc = sample_grid(e, k))) return rc;
    if (m) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_sample_points, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, (const float4*)e->d_sPV, e->d_cellStart,
                           reinterpret_cast<const float4*>(devPoints4), (void*)devOut, m);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_sample_points(SphEngine* e, const float* points4, size_t m, SphSample* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (m && (!points4 || !out)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = query_refused(e))) return rc;                                         // (the refusal, before any allocation)
    if (m && ((rc = e->d_sampleIn.grow(e, m)) || (rc = e->d_sampleOut.grow(e, m)))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = sph_sample_points_device(e, reinterpret_cast<const float*>(e->d_sampleIn.p), m, e->d_sampleOut.p))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(out, e->d_sampleOut.p, m * sizeof(SphSample), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_sample_lattice(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int field, void* devOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!origin || !spacing || !dims || !devOut) return fail(SPH_ERR_ARG, "null argument");
    if (field < SPH_FIELD_DENSITY || field > SPH_FIELD_ALL) return fail(SPH_ERR_ARG, "unknown field %d", field);
    SimK k;
    int rc;
    if ((rc = check_lattice(dims, spacing, 1, nullptr)) || (rc = sample_grid(e, k))) return rc;
    const LatticeK L = lattice_consts(origin, spacing, dims, field, kSampleStage);
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_sample_lattice, dim3((unsigned)std::min<long long>(L.nBricks, 1ll << 20)), dim3(kBlock), 0, e->stream, k, L,
                           (const float4*)e->d_sPV, e->d_cellStart, devOut);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

// ---- neighbour lists (sph_neighbors.h) -----------------------------------------------------------
static_assert(sizeof(SphNeighborInfo) == 40, "SphNeighborInfo must be 40 bytes");
static_assert(sizeof(long long) == sizeof(int64_t), "offsets are int64");

// Radius and flags as arguments: the stencil half-width through *stencil.
static int neighbors_check(float radius, float cellSize, int flags, bool query, int* stencil) {
    if (flags & ~(SPH_NEIGHBORS_SELF | SPH_NEIGHBORS_HALF | SPH_NEIGHBORS_COUNT_ONLY)) return fail(SPH_ERR_ARG, "unknown neighbour flags %d", flags);
    if ((flags & SPH_NEIGHBORS_SELF) && (flags & SPH_NEIGHBORS_HALF)) return fail(SPH_ERR_ARG, "SPH_NEIGHBORS_SELF | SPH_NEIGHBORS_HALF: a half list has no diagonal");
    if (query && (flags & (SPH_NEIGHBORS_SELF | SPH_NEIGHBORS_HALF))) return fail(SPH_ERR_ARG, "SPH_NEIGHBORS_SELF / _HALF apply to particle lists only");
    return radius_stencil(radius, cellSize, stencil);
}

// Grid of the current state, ids, count, scan, one synchronisation for the total, then the fill (arguments already checked for null).
static int neighbors_run(SphEngine* e, const float4* devPoints, size_t m, float radius, int flags, uint64_t maxPairs, SphNeighborInfo* out) {
    using namespace sph;
    const bool query = devPoints != nullptr || m != 0;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = neighbors_check(radius, g.cellSize, flags, query, &stencil))) return rc;
    const size_t n = e->n, rows = query ? m : n;
    e->nbInfo = SphNeighborInfo{};                                                  // (the lists held so far end here)
    e->nbIndexed = false;
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_nbCnt.grow(e, rows)) || (rc = e->d_nbOffsets.grow(e, rows + 1)) ||
        (rc = e->scanScratch.grow(e, rows))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, radius, stencil, flags, e->n);
    const dim3 grid(blocks_for(rows)), block(kBlock);
    using Count = void (*)(SimK, NbK, const float4*, const uint32_t*, const int32_t*, const float4*, size_t, uint32_t*);
    using Fill = void (*)(SimK, NbK, const float4*, const uint32_t*, const int32_t*, const float4*, size_t, const long long*, int32_t*);
    auto walk = [&](bool fill) {
        Timed t(e, SPH_K_OTHER);
        auto go = [&](auto kernel, auto... own) {                                   // the arguments every walk shares, then the kernel's own
            hipLaunchKernelGGL(kernel, grid, block, 0, e->stream, k, nb, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const int32_t*)e->d_slotIds.p, devPoints, rows, own...);
        };
        if (!fill) return go(query ? (Count)k_neighbors_count<false> : (Count)k_neighbors_count<true>, e->d_nbCnt.p);
        const Fill plain = query ? (Fill)k_neighbors_fill<false> : (Fill)k_neighbors_fill<true>, wave = query ? (Fill)k_neighbors_fill_wave<false> : (Fill)k_neighbors_fill_wave<true>;
        go(e->optNbFill ? wave : plain, (const long long*)e->d_nbOffsets.p, e->d_nbIndices.p);
    };
    unsigned long long host[2] = {0ull, 0ull};
    if (rows) {
        slot_ids_fill(e);
        walk(false);                                                                // (writes cnt[row] of every row)
        if ((rc = scan_counts64(e, e->d_nbCnt.p, rows, e->d_nbOffsets.p, host))) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(e->d_nbOffsets.p, 0, sizeof(long long), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    SphNeighborInfo info{};
    info.rows = rows; info.total = host[0]; info.radius = radius; info.stencil = stencil; info.flags = flags; info.kind = query ? 2 : 1;
    info.maxCount = (uint32_t)host[1];
    e->nbInfo = info;
    if (out) *out = info;
    if (maxPairs && info.total > maxPairs)
        return fail(SPH_ERR_CAPACITY, "%llu neighbour pairs exceed maxPairs %llu (offsets are valid, no indices were written)", (unsigned long long)info.total, (unsigned long long)maxPairs);
    if (flags & SPH_NEIGHBORS_COUNT_ONLY) return SPH_OK;
    if ((rc = e->d_nbIndices.grow(e, (size_t)info.total))) return rc;
    if (rows && info.total) walk(true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->nbIndexed = true;
    return SPH_OK;
}

int sph_neighbors_build(SphEngine* e, float radius, int flags, uint64_t maxPairs, SphNeighborInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    return neighbors_run(e, nullptr, 0, radius, flags, maxPairs, out);
}

int sph_neighbors_query(SphEngine* e, const float* devPoints4, size_t m, float radius, int flags, uint64_t maxPairs, SphNeighborInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || !devPoints4) return fail(SPH_ERR_ARG, "null argument");
    if (m == 0 || m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (1 .. 2^31 - 1)", m);
    return neighbors_run(e, reinterpret_cast<const float4*>(devPoints4), m, radius, flags, maxPairs, out);
}

int sph_neighbors_info(const SphEngine* e, SphNeighborInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->nbInfo;
    return SPH_OK;
}

int sph_neighbors_device(SphEngine* e, const int64_t** offsets, const int32_t** indices) {
    if (!e || !offsets || !indices) return fail(SPH_ERR_ARG, "null argument");
    if (!e->nbInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no neighbour lists");
    *offsets = reinterpret_cast<const int64_t*>(e->d_nbOffsets.p);
    *indices = e->nbIndexed ? e->d_nbIndices.p : nullptr;
    return SPH_OK;
}

static int neighbors_copy(SphEngine* e, int64_t* offsets, int32_t* indices, uint64_t indexCap, hipMemcpyKind kind) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!offsets || (e->nbIndexed && e->nbInfo.total && !indices)) return fail(SPH_ERR_ARG, "null argument");
    if (!e->nbInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no neighbour lists");
    if (e->nbIndexed && indexCap < e->nbInfo.total)
        return fail(SPH_ERR_CAPACITY, "room for %llu indices, the lists hold %llu", (unsigned long long)indexCap, (unsigned long long)e->nbInfo.total);
    HIP_TRY(hipMemcpyAsync(offsets, e->d_nbOffsets.p, ((size_t)e->nbInfo.rows + 1) * sizeof(int64_t), kind, e->stream));
    if (e->nbIndexed && e->nbInfo.total) HIP_TRY(hipMemcpyAsync(indices, e->d_nbIndices.p, (size_t)e->nbInfo.total * sizeof(int32_t), kind, e->stream));
    return SPH_OK;
}
int sph_neighbors_export(SphEngine* e, int64_t* devOffsets, int32_t* devIndices, uint64_t indexCap) {
    return neighbors_copy(e, devOffsets, devIndices, indexCap, hipMemcpyDeviceToDevice);
}
int sph_neighbors_download(SphEngine* e, int64_t* offsets, int32_t* indices, uint64_t indexCap) {
    int rc;
    if ((rc = neighbors_copy(e, offsets, indices, indexCap, hipMemcpyDeviceToHost))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_neighbors_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m,
                       float radius, int flags, int64_t* offsets, int32_t* indices, uint64_t indexCap, SphNeighborInfo* out) {
    if (!params || !offsets || !out || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    int rc, stencil = 0;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = neighbors_check(radius, g.cellSize, flags, query, &stencil))) return rc;
    const float R2 = radius * radius;
    const sph::HostGrid grid(k, particles, n);
    const std::vector<uint32_t>& order = grid.order;
    const std::vector<uint32_t>& slotOf = grid.slotOf;
    const size_t rows = query ? m : n;
    // f(id) per kept entry of row r, in order
    auto walk = [&](size_t r, auto&& f) {
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        if (query && !(sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2]))) return;
        grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                const float* y = particles[order[j]].pos;
                const bool acc = sph::neighbor_accept(x[0], x[1], x[2], y[0], y[1], y[2], R2);
                if (query ? acc : sph::neighbor_keep(flags, j == slotOf[r], acc, (uint32_t)r, order[j])) f(order[j]);
            }
        });
    };
    uint64_t total = 0;
    uint32_t maxCount = 0;
    for (size_t r = 0; r < rows; ++r) {
        uint32_t c = 0;
        offsets[r] = (int64_t)total;
        walk(r, [&](uint32_t) { c += 1u; });
        total += c;
        maxCount = std::max(maxCount, c);
    }
    offsets[rows] = (int64_t)total;
    SphNeighborInfo info{};
    info.rows = rows; info.total = total; info.radius = radius; info.stencil = stencil; info.flags = flags; info.kind = query ? 2 : 1;
    info.maxCount = maxCount;
    *out = info;
    if (flags & SPH_NEIGHBORS_COUNT_ONLY) return SPH_OK;
    if (total > indexCap) return fail(SPH_ERR_CAPACITY, "room for %llu indices, the lists hold %llu", (unsigned long long)indexCap, (unsigned long long)total);
    if (total && !indices) return fail(SPH_ERR_ARG, "null argument");
    for (size_t r = 0; r < rows; ++r) {
        int64_t w = offsets[r];
        walk(r, [&](uint32_t id) { indices[w++] = (int32_t)id; });
    }
    return SPH_OK;
}

// ---- connected components (sph_components.h) -----------------------------------------------------
static_assert(sizeof(SphComponent) == 64 && sizeof(SphComponent) == sizeof(sph::CcRow), "SphComponent must be 64 bytes");
static_assert(offsetof(SphComponent, bbMin) == offsetof(sph::CcRow, bbMin) && offsetof(SphComponent, sumQ) == offsetof(sph::CcRow, sumQ) &&
              offsetof(SphComponent, flags) == offsetof(sph::CcRow, flags), "CcRow is the device view of SphComponent");
static_assert(sizeof(SphComponentInfo) == 56, "SphComponentInfo must be 56 bytes");

static int components_check(float radius, float cellSize, int flags, int* stencil) {
    if (flags & ~SPH_COMPONENTS_FLUID_ONLY) return fail(SPH_ERR_ARG, "unknown component flags %d", flags);
    return radius_stencil(radius, cellSize, stencil);
}

int sph_components_build(SphEngine* e, float radius, int flags, SphComponentInfo* out) {
    using namespace sph;
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = components_check(radius, g.cellSize, flags, &stencil))) return rc;
    const size_t n = e->n;
    e->ccInfo = SphComponentInfo{};                                                 // (the result held so far ends here)
    e->ccValid = false;
    if ((rc = e->d_ccIds.grow(e, n)) || (rc = e->d_ccLabels.grow(e, n)) || (rc = e->d_ccRoots.grow(e, n)) || (rc = e->d_ccParent.grow(e, n)) ||
        (rc = e->d_ccMinId.grow(e, n)) || (rc = e->d_ccFlag.grow(e, n)) || (rc = e->d_ccOffsets.grow(e, n + 1)) || (rc = e->scanScratch.grow(e, n)) ||
        (rc = e->d_ccWords.grow(e, (size_t)kCcWords)) || (rc = e->d_ccStats.grow(e, 3))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    SphComponentInfo info{};
    info.rows = n; info.radius = radius; info.stencil = stencil; info.flags = flags;
    uint64_t C = 0;
    if (n) {
        const NbK nb = make_nbk(e, radius, stencil, flags, e->n);
        const dim3 grid(blocks_for(n)), block(kBlock);
        const float4* pv = (const float4*)e->d_sPV;
        const uint32_t* cellStart = (const uint32_t*)e->d_cellStart;
        const int32_t* ids = e->d_ccIds.p;
        uint32_t* parent = e->d_ccParent.p;
        uint32_t* words = e->d_ccWords.p;
        HIP_TRY(hipMemsetAsync(words, 0, (size_t)kCcWords * sizeof(uint32_t), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_ccStats.p, 0, 3 * sizeof(unsigned long long), e->stream));
        {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_components_init, grid, block, 0, e->stream, (const float4*)e->d_sOwn, e->d_ccIds.p, parent, e->d_ccMinId.p, e->idBase, (uint32_t)n, flags);
        }
        // hook + compress until a whole hook launch finds every edge inside one tree; every launch has a word of its own
        int word = 0;
        auto compress = [&]() {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_components_compress, grid, block, 0, e->stream, parent, (uint32_t)n, words + word);
            return word++;
        };
        bool done = false;
        uint32_t rounds = 0;
        while (!done && rounds < (uint32_t)kCcMaxRounds) {
            const int hookWord = word++;
            {
                Timed t(e, SPH_K_OTHER);
                if (e->optCcVariant & kCcFullWalk) hipLaunchKernelGGL((k_components_hook<false>), grid, block, 0, e->stream, k, nb, pv, cellStart, ids, parent, words + hookWord);
                else hipLaunchKernelGGL((k_components_hook<true>), grid, block, 0, e->stream, k, nb, pv, cellStart, ids, parent, words + hookWord);
            }
            rounds += 1;
            int jumpWord = compress();                                              // (queued before the hook's word is known: one round trip per round)
            uint32_t got[2] = {0u, 0u};                                             // the hook's "changed", the compress launch's "more"
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(got, words + hookWord, sizeof(got), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (!got[0]) { done = true; break; }
            for (int jumps = 1; got[1]; ++jumps) {
                if (jumps >= kCcMaxJumps) return fail(SPH_ERR_STATE, "components: the trees were not flat after %d compress launches in round %u", jumps, rounds);
                jumpWord = compress();
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(got + 1, words + jumpWord, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
                HIP_TRY(hipStreamSynchronize(e->stream));
            }
        }
        if (!done) return fail(SPH_ERR_STATE, "components: no hook launch found every edge inside one tree within %u rounds", rounds);
        info.rounds = rounds;
        {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_components_minid, grid, block, 0, e->stream, ids, (const uint32_t*)parent, e->d_ccMinId.p, (uint32_t)n);
        }
        {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_components_roots, grid, block, 0, e->stream, ids, (const uint32_t*)parent, (const uint32_t*)e->d_ccMinId.p, e->d_ccRoots.p, e->d_ccFlag.p, (uint32_t)n);
        }
        unsigned long long host[2] = {0ull, 0ull};
        if ((rc = scan_counts64(e, e->d_ccFlag.p, n, e->d_ccOffsets.p, host))) return rc;
        C = host[0];
        if (C > n) return fail(SPH_ERR_STATE, "components: %llu bodies of %zu records", (unsigned long long)C, n);
        if ((rc = e->d_ccTable.grow(e, (size_t)C))) return rc;
        const double S = 65536.0 / (double)k.cellSize;
        if (C) {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_components_table_init, dim3(blocks_for((size_t)C)), block, 0, e->stream, e->d_ccTable.p, (uint32_t)C);
        }
        {
            Timed t(e, SPH_K_OTHER);                                                // (with C == 0 it still writes the labels: all -1)
            if (e->optCcVariant & kCcLaneAtomics) hipLaunchKernelGGL((k_components_label<false>), grid, block, 0, e->stream, k, S, pv, ids, (const int32_t*)e->d_ccRoots.p, (const long long*)e->d_ccOffsets.p, e->d_ccLabels.p, e->d_ccTable.p, (uint32_t)n, (uint32_t)C);
            else hipLaunchKernelGGL((k_components_label<true>), grid, block, 0, e->stream, k, S, pv, ids, (const int32_t*)e->d_ccRoots.p, (const long long*)e->d_ccOffsets.p, e->d_ccLabels.p, e->d_ccTable.p, (uint32_t)n, (uint32_t)C);
        }
        unsigned long long stats[3] = {0ull, 0ull, 0ull};
        if (C) {
            {
                Timed t(e, SPH_K_OTHER);
                hipLaunchKernelGGL(k_components_finish, dim3(blocks_for((size_t)C)), block, 0, e->stream, e->d_ccTable.p, (uint32_t)C, e->d_ccStats.p);
            }
            HIP_TRY(hipMemcpyAsync(stats, e->d_ccStats.p, sizeof(stats), hipMemcpyDeviceToHost, e->stream));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream));
        info.numComponents = C;
        info.numExcluded = n - stats[2];
        if (C) {
            info.largestCount = stats[0] >> 32;
            info.largestRoot = ~(uint32_t)(stats[0] & 0xffffffffull);
            info.numSingletons = (uint32_t)stats[1];
        }
    }
    e->ccInfo = info;
    e->ccValid = true;
    *out = info;
    return SPH_OK;
}

int sph_components_info(const SphEngine* e, SphComponentInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->ccValid) return fail(SPH_ERR_STATE, "the engine holds no components");
    *out = e->ccInfo;
    return SPH_OK;
}

int sph_components_device(SphEngine* e, const int32_t** labels, const int32_t** roots, const SphComponent** table) {
    if (!e || !labels || !roots || !table) return fail(SPH_ERR_ARG, "null argument");
    if (!e->ccValid) return fail(SPH_ERR_STATE, "the engine holds no components");
    *labels = e->d_ccLabels.p;
    *roots = e->d_ccRoots.p;
    *table = reinterpret_cast<const SphComponent*>(e->d_ccTable.p);
    return SPH_OK;
}

int sph_components_download(SphEngine* e, int32_t* labels, int32_t* roots, SphComponent* table, uint64_t tableCap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->ccValid) return fail(SPH_ERR_STATE, "the engine holds no components");
    const size_t n = (size_t)e->ccInfo.rows, C = (size_t)e->ccInfo.numComponents;
    if (table && tableCap < C) return fail(SPH_ERR_CAPACITY, "room for %llu table rows, the engine holds %zu components", (unsigned long long)tableCap, C);
    if (labels && n) HIP_TRY(hipMemcpyAsync(labels, e->d_ccLabels.p, n * sizeof(int32_t), hipMemcpyDefault, e->stream));
    if (roots && n) HIP_TRY(hipMemcpyAsync(roots, e->d_ccRoots.p, n * sizeof(int32_t), hipMemcpyDefault, e->stream));
    if (table && C) HIP_TRY(hipMemcpyAsync(table, e->d_ccTable.p, C * sizeof(SphComponent), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_components_host(const SphParticle* particles, size_t n, const SphParams* params, float radius, int flags,
                        int32_t* labels, int32_t* roots, SphComponent* table, uint64_t tableCap, SphComponentInfo* out) {
    if (!params || !out || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    int rc, stencil = 0;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = components_check(radius, g.cellSize, flags, &stencil))) return rc;
    const float R2 = radius * radius;
    const bool fluidOnly = (flags & SPH_COMPONENTS_FLUID_ONLY) != 0;
    const sph::HostGrid grid(k, particles, n);
    const std::vector<uint32_t>& order = grid.order;
    const std::vector<uint32_t>& slotOf = grid.slotOf;
    // a plain sequential union-find over particle ids: the smaller root wins, so a root is the smallest id of its tree
    std::vector<uint32_t> parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        uint32_t r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) { const uint32_t nx = parent[x]; parent[x] = r; x = nx; }
        return r;
    };
    auto takesPart = [&](size_t i) { return !(fluidOnly && particles[i].isGhost != 0); };
    for (size_t i = 0; i < n; ++i) {
        if (!takesPart(i)) continue;
        const float* x = particles[i].pos;
        grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe && j < slotOf[i]; ++j) {                   // an edge is seen from its larger slot
                const uint32_t o = order[j];
                const float* y = particles[o].pos;
                if (!takesPart(o) || !sph::neighbor_accept(x[0], x[1], x[2], y[0], y[1], y[2], R2)) continue;
                const uint32_t a = find((uint32_t)i), b = find(o);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            }
        });
    }
    std::vector<int32_t> lab(n, -1), root(n, -1);
    std::vector<sph::CcRow> rows;
    uint64_t excluded = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!takesPart(i)) { excluded += 1; continue; }
        const uint32_t r = find((uint32_t)i);                                       // r <= i: its row exists already
        root[i] = (int32_t)r;
        if (r == i) {
            sph::CcRow row{};
            row.root = r;
            for (int a = 0; a < 3; ++a) { row.bbMin[a] = 0xffffffffu; row.bbMax[a] = 0u; }
            lab[i] = (int32_t)rows.size();
            rows.push_back(row);
        } else {
            lab[i] = lab[r];
        }
        sph::CcRow& row = rows[(size_t)lab[i]];
        row.count += 1u;
        const float* x = particles[i].pos;
        if (!sph::cc_finite3(x[0], x[1], x[2])) { row.flags |= sph::kCcNonFinite; continue; }
        const float gmin[3] = {k.gminx, k.gminy, k.gminz};
        const double S = 65536.0 / (double)k.cellSize;
        for (int a = 0; a < 3; ++a) {
            row.sumQ[a] += (unsigned long long)sph::cc_fixed(x[a], gmin[a], S);
            row.bbMin[a] = std::min(row.bbMin[a], sph::cc_ordered(x[a]));
            row.bbMax[a] = std::max(row.bbMax[a], sph::cc_ordered(x[a]));
        }
    }
    SphComponentInfo info{};
    info.rows = n; info.numComponents = rows.size(); info.numExcluded = excluded; info.radius = radius; info.stencil = stencil; info.flags = flags;
    for (sph::CcRow& row : rows) {
        const bool empty = (row.flags & sph::kCcNonFinite) != 0u;
        for (int a = 0; a < 3; ++a) {
            const float mn = empty ? 0.0f : sph::cc_unordered(row.bbMin[a]), mx = empty ? 0.0f : sph::cc_unordered(row.bbMax[a]);
            memcpy(&row.bbMin[a], &mn, 4);
            memcpy(&row.bbMax[a], &mx, 4);
        }
        if (row.count > info.largestCount) { info.largestCount = row.count; info.largestRoot = row.root; }     // (rows ascend by root: ties keep the smaller)
        if (row.count == 1u) info.numSingletons += 1u;
    }
    *out = info;
    if (table && tableCap < rows.size())
        return fail(SPH_ERR_CAPACITY, "room for %llu table rows, the state has %zu components", (unsigned long long)tableCap, rows.size());
    if (labels && n) memcpy(labels, lab.data(), n * sizeof(int32_t));
    if (roots && n) memcpy(roots, root.data(), n * sizeof(int32_t));
    if (table && !rows.empty()) memcpy(table, rows.data(), rows.size() * sizeof(SphComponent));
    return SPH_OK;
}

// ---- k nearest neighbours (sph_knn.h) --------------------------------------------------------------
static_assert(sizeof(SphKnnInfo) == 48, "SphKnnInfo must be 48 bytes");
static_assert(SPH_KNN_SELF == sph::kKnnSelf && SPH_KNN_FLUID_ONLY == sph::kKnnFluidOnly && SPH_KNN_MAX_K == sph::kKnnMaxK, "sph_knn.h mirrors SPH_KNN_*");

static int knn_check(int k, float radius, float cellSize, int flags, bool query, int* stencil) {
    if (flags & ~(SPH_KNN_SELF | SPH_KNN_FLUID_ONLY)) return fail(SPH_ERR_ARG, "unknown kNN flags %d", flags);
    if (query && (flags & SPH_KNN_SELF)) return fail(SPH_ERR_ARG, "SPH_KNN_SELF applies to particle rows only");
    if (k < 1 || k > SPH_KNN_MAX_K) return fail(SPH_ERR_ARG, "k = %d (1 .. %d)", k, (int)SPH_KNN_MAX_K);
    return radius_stencil(radius, cellSize, stencil);
}

// One launch of the variant and class in force (arguments already checked).
static void knn_launch(SphEngine* e, bool query, const sph::SimK& k, const sph::NbK& nb, int kk, const float4* devPoints, size_t rows) {
    using namespace sph;
    using Kernel = void (*)(SimK, NbK, int, const float4*, const uint32_t*, const int32_t*, const float4*, const float4*, size_t, int32_t*, float*, uint32_t*,
                            unsigned long long*);
    auto go = [&](Kernel kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(blocks_for(rows, threads)), dim3(threads), 0, e->stream, k, nb, kk, (const float4*)e->d_sPV,
                           (const uint32_t*)e->d_cellStart, (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn, devPoints, rows, e->d_knnIndices.p,
                           e->d_knnDist2.p, e->d_knnCounts.p, e->d_knnStats.p);
    };
    if (e->optKnnVariant == 1) return go(query ? k_knn_select<false> : k_knn_select<true>, kBlock);
    switch (knn_class(kk)) {
    case 8: return go(query ? k_knn<false, 8> : k_knn<true, 8>, knn_threads(8));
    case 16: return go(query ? k_knn<false, 16> : k_knn<true, 16>, knn_threads(16));
    case 32: return go(query ? k_knn<false, 32> : k_knn<true, 32>, knn_threads(32));
    default: return go(query ? k_knn<false, 64> : k_knn<true, 64>, knn_threads(64));
    }
}

// Grid of the current state, ids, the selection, one synchronisation for the two totals.
static int knn_run(SphEngine* e, bool query, const float4* devPoints, size_t m, int kk, float radius, int flags, SphKnnInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = knn_check(kk, radius, g.cellSize, flags, query, &stencil))) return rc;
    const size_t n = e->n, rows = query ? m : n;
    e->knnInfo = SphKnnInfo{};                                                      // (the rows held so far end here)
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_knnIndices.grow(e, rows * (size_t)kk)) || (rc = e->d_knnDist2.grow(e, rows * (size_t)kk)) ||
        (rc = e->d_knnCounts.grow(e, rows)) || (rc = e->d_knnStats.grow(e, 2))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, radius, stencil, flags, e->n);
    unsigned long long host[2] = {0ull, 0ull};
    if (rows) {
        HIP_TRY(hipMemsetAsync(e->d_knnStats.p, 0, 2 * sizeof(unsigned long long), e->stream));
        slot_ids_fill(e);
        {
            Timed t(e, SPH_K_OTHER);
            knn_launch(e, query, k, nb, kk, devPoints, rows);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, e->d_knnStats.p, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    SphKnnInfo info{};
    info.rows = rows; info.total = host[0]; info.rowsFull = host[1]; info.radius = radius; info.k = kk; info.stencil = stencil; info.flags = flags;
    info.kind = query ? 2 : 1;
    e->knnInfo = info;
    *out = info;
    return SPH_OK;
}

int sph_knn_build(SphEngine* e, int k, float radius, int flags, SphKnnInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    return knn_run(e, false, nullptr, 0, k, radius, flags, out);
}

int sph_knn_query(SphEngine* e, const float* devPoints4, size_t m, int k, float radius, int flags, SphKnnInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || (m && !devPoints4)) return fail(SPH_ERR_ARG, "null argument");
    if (m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    return knn_run(e, true, reinterpret_cast<const float4*>(devPoints4), m, k, radius, flags, out);
}

int sph_knn_info(const SphEngine* e, SphKnnInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->knnInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no k nearest neighbours");
    *out = e->knnInfo;
    return SPH_OK;
}

int sph_knn_device(SphEngine* e, const int32_t** indices, const float** dist2, const uint32_t** counts) {
    if (!e || !indices || !dist2 || !counts) return fail(SPH_ERR_ARG, "null argument");
    if (!e->knnInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no k nearest neighbours");
    *indices = e->d_knnIndices.p;
    *dist2 = e->d_knnDist2.p;
    *counts = e->d_knnCounts.p;
    return SPH_OK;
}

int sph_knn_download(SphEngine* e, int32_t* indices, float* dist2, uint32_t* counts) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->knnInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no k nearest neighbours");
    const size_t rows = (size_t)e->knnInfo.rows, cells = rows * (size_t)e->knnInfo.k;
    if (indices && cells) HIP_TRY(hipMemcpyAsync(indices, e->d_knnIndices.p, cells * sizeof(int32_t), hipMemcpyDefault, e->stream));
    if (dist2 && cells) HIP_TRY(hipMemcpyAsync(dist2, e->d_knnDist2.p, cells * sizeof(float), hipMemcpyDefault, e->stream));
    if (counts && rows) HIP_TRY(hipMemcpyAsync(counts, e->d_knnCounts.p, rows * sizeof(uint32_t), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_knn_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m, int kk, float radius, int flags,
                 int32_t* indices, float* dist2, uint32_t* counts, SphKnnInfo* out) {
    if (!params || !out || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    int rc, stencil = 0;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = knn_check(kk, radius, g.cellSize, flags, query, &stencil))) return rc;
    const float R2 = radius * radius;
    const bool self = (flags & SPH_KNN_SELF) != 0, fluidOnly = (flags & SPH_KNN_FLUID_ONLY) != 0;
    const sph::HostGrid grid(k, particles, n);
    const std::vector<uint32_t>& order = grid.order;
    const std::vector<uint32_t>& slotOf = grid.slotOf;
    const size_t rows = query ? m : n;
    SphKnnInfo info{};
    info.rows = rows; info.radius = radius; info.k = kk; info.stencil = stencil; info.flags = flags; info.kind = query ? 2 : 1;
    std::vector<unsigned long long> keys;
    for (size_t r = 0; r < rows; ++r) {
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        keys.clear();
        const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
        if (walk) {
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    if (!query && !self && j == slotOf[r]) continue;
                    const uint32_t o = order[j];
                    const float* y = particles[o].pos;
                    const float r2 = sph::knn_r2(x[0], x[1], x[2], y[0], y[1], y[2]);
                    if (!(r2 < R2) || (fluidOnly && particles[o].isGhost != 0)) continue;
                    keys.push_back(sph::knn_key(r2, o));
                }
            });
        }
        std::sort(keys.begin(), keys.end());
        const size_t c = std::min(keys.size(), (size_t)kk);
        for (size_t s = 0; s < (size_t)kk; ++s) {
            if (indices) indices[r * (size_t)kk + s] = s < c ? (int32_t)(uint32_t)(keys[s] & 0xffffffffull) : -1;
            if (dist2) dist2[r * (size_t)kk + s] = s < c ? sph::knn_key_r2(keys[s]) : INFINITY;
        }
        if (counts) counts[r] = (uint32_t)c;
        info.total += c;
        info.rowsFull += c == (size_t)kk ? 1u : 0u;
    }
    *out = info;
    return SPH_OK;
}

// ---- free-surface particles (sph_shell.h) ------------------------------------------------------------
static_assert(sizeof(SphShell) == 32 && sizeof(SphShellConfig) == 16 && sizeof(SphShellInfo) == 48, "SphShell is 32 bytes, SphShellConfig 16, SphShellInfo 48");
static_assert(sizeof(sph::ShellRow) == sizeof(SphShell) && offsetof(sph::ShellRow, crest) == offsetof(SphShell, crest) &&
              offsetof(sph::ShellRow, flags) == offsetof(SphShell, flags), "sph_shell.h mirrors SphShell");
static_assert(SPH_SHELL_FLUID_ONLY == sph::kShellFluidOnly && SPH_SHELL_MEMBER == sph::kShellMember && SPH_SHELL_ISOLATED == sph::kShellIsolated,
              "sph_shell.h mirrors SPH_SHELL_*");

void sph_shell_default(SphShellConfig* cfg) {
    if (!cfg) return;
    cfg->radius = 0.0f; cfg->offset = 0.10f; cfg->minCount = 0u; cfg->flags = 0;
}

// The config as an argument: *radius is the radius in force (cfg.radius <= 0: h), the stencil half-width through *stencil.
static int shell_check(const SphShellConfig& cfg, float h, float cellSize, float* radius, int* stencil) {
    if (cfg.flags & ~SPH_SHELL_FLUID_ONLY) return fail(SPH_ERR_ARG, "unknown shell flags %d", cfg.flags);
    if (!std::isfinite(cfg.offset) || cfg.offset < 0.0f) return fail(SPH_ERR_ARG, "offset %g is not finite or < 0", (double)cfg.offset);
    *radius = shell_radius(cfg, h);
    return radius_stencil(*radius, cellSize, stencil);
}

// Grid of the current state, ids, pass 1, the scan of the flags by row (ids) and -- particle rows -- by slot (the targets of pass 2), pass 2.
// One synchronisation in the middle, for numShell (it sizes pass 2) and the two words of the reduction, and the one that ends the call.
static int shell_run(SphEngine* e, bool query, const float4* devPoints, size_t m, const SphShellConfig& cfg, SphShellInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    float radius = 0.0f;
    if ((rc = query_grid(e, g)) || (rc = shell_check(cfg, e->params.param_h, g.cellSize, &radius, &stencil))) return rc;
    const size_t n = e->n, rows = query ? m : n;
    e->shellInfo = SphShellInfo{};                                                  // (the rows held so far end here)
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_shRows.grow(e, rows)) || (rc = e->d_shIds.grow(e, rows)) || (rc = e->d_shFlagRow.grow(e, rows)) ||
        (rc = e->d_shOffsets.grow(e, rows + 1)) || (rc = e->scanScratch.grow(e, rows)) ||
        (rc = e->d_shStats.grow(e, 2))) return rc;
    if (!query && ((rc = e->d_shNrm.grow(e, n)) || (rc = e->d_shFlagSlot.grow(e, n)) || (rc = e->d_shSlots.grow(e, n)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, radius, stencil, cfg.flags, e->n);
    const ShellK sk = shell_consts(cfg, radius);
    const int timed = e->optShellTimed;
    unsigned long long stats[2] = {0ull, 0ull}, totals[2] = {0ull, 0ull};
    if (rows) {
        const dim3 grid(blocks_for(rows)), block(kBlock);
        const float4* pv = (const float4*)e->d_sPV;
        const uint32_t* cellStart = (const uint32_t*)e->d_cellStart;
        HIP_TRY(hipMemsetAsync(e->d_shStats.p, 0, 2 * sizeof(unsigned long long), e->stream));
        std::unique_ptr<Timed> t;
        auto bracket = [&](int part) { t.reset(); if (timed == 0 || timed == part) t.reset(new Timed(e, SPH_K_OTHER)); };
        if (timed == 0 || timed == 1) slot_ids_fill(e);
        else if (n) hipLaunchKernelGGL(k_neighbors_ids, dim3(blocks_for(n)), block, 0, e->stream, (const float4*)e->d_sOwn, e->d_slotIds.p, e->idBase, (uint32_t)n);
        bracket(1);
        if (query) hipLaunchKernelGGL((k_shell_gather<false>), grid, block, 0, e->stream, k, nb, sk, pv, cellStart, (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn,
                                      devPoints, rows, e->d_shRows.p, e->d_shFlagRow.p, (float4*)nullptr, (uint32_t*)nullptr, e->d_shStats.p);
        else hipLaunchKernelGGL((k_shell_gather<true>), grid, block, 0, e->stream, k, nb, sk, pv, cellStart, (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn,
                                devPoints, rows, e->d_shRows.p, e->d_shFlagRow.p, e->d_shNrm.p, e->d_shFlagSlot.p, e->d_shStats.p);
        bracket(3);                                                                 // ids[]: the flags by row, scanned and compacted
        unsigned long long* devTotals = scan_counts64_launch(e, e->scanScratch, e->d_shFlagRow.p, rows, e->d_shOffsets.p);
        hipLaunchKernelGGL(k_shell_compact, grid, block, 0, e->stream, (const uint32_t*)e->d_shFlagRow.p, (const long long*)e->d_shOffsets.p, rows, e->d_shIds.p);
        t.reset();
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(totals, devTotals, sizeof(totals), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(stats, e->d_shStats.p, sizeof(stats), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const size_t numShell = (size_t)totals[0];
        if (numShell > rows) return fail(SPH_ERR_STATE, "shell: %zu shell rows of %zu", numShell, rows);
        if (!query && numShell) {                                                   // the same scan by slot: pass 2's targets in ascending slot order
            bracket(3);
            (void)scan_counts64_launch(e, e->scanScratch, e->d_shFlagSlot.p, n, e->d_shOffsets.p);
            hipLaunchKernelGGL(k_shell_compact, grid, block, 0, e->stream, (const uint32_t*)e->d_shFlagSlot.p, (const long long*)e->d_shOffsets.p, n, e->d_shSlots.p);
            bracket(2);
            hipLaunchKernelGGL(k_shell_crest, dim3(blocks_for(numShell)), block, 0, e->stream, k, nb, sk, pv, cellStart, (const int32_t*)e->d_slotIds.p,
                               (const float4*)e->d_shNrm.p, (const int32_t*)e->d_shSlots.p, numShell, rows, e->d_shRows.p);
            t.reset();
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    SphShellInfo info{};
    info.rows = rows; info.numShell = totals[0]; info.numIsolated = stats[0]; info.maxCount = (uint32_t)stats[1]; info.radius = radius;
    info.stencil = stencil; info.kind = query ? 2 : 1; info.flags = cfg.flags;
    e->shellInfo = info;
    *out = info;
    return SPH_OK;
}

int sph_shell_build(SphEngine* e, const SphShellConfig* cfg, SphShellInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !out) return fail(SPH_ERR_ARG, "null argument");
    return shell_run(e, false, nullptr, 0, *cfg, out);
}

int sph_shell_query(SphEngine* e, const float* devPoints4, size_t m, const SphShellConfig* cfg, SphShellInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !out || (m && !devPoints4)) return fail(SPH_ERR_ARG, "null argument");
    if (m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    return shell_run(e, true, reinterpret_cast<const float4*>(devPoints4), m, *cfg, out);
}

int sph_shell_info(const SphEngine* e, SphShellInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->shellInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no free-surface rows");
    *out = e->shellInfo;
    return SPH_OK;
}

int sph_shell_device(SphEngine* e, const SphShell** rows, const int32_t** ids) {
    if (!e || !rows || !ids) return fail(SPH_ERR_ARG, "null argument");
    if (!e->shellInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no free-surface rows");
    *rows = reinterpret_cast<const SphShell*>(e->d_shRows.p);
    *ids = e->d_shIds.p;
    return SPH_OK;
}

int sph_shell_download(SphEngine* e, SphShell* rows, int32_t* ids) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->shellInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no free-surface rows");
    const size_t r = (size_t)e->shellInfo.rows, s = (size_t)e->shellInfo.numShell;
    if (rows && r) HIP_TRY(hipMemcpyAsync(rows, e->d_shRows.p, r * sizeof(SphShell), hipMemcpyDefault, e->stream));
    if (ids && s) HIP_TRY(hipMemcpyAsync(ids, e->d_shIds.p, s * sizeof(int32_t), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_shell_host(const SphParticle* particles, size_t n, const SphParams* params, const float* points4, size_t m, const SphShellConfig* cfg,
                   SphShell* rowsOut, int32_t* ids, float* sums4, SphShellInfo* out) {
    if (!params || !cfg || !out || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    int rc, stencil = 0;
    float radius = 0.0f;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = shell_check(*cfg, params->param_h, g.cellSize, &radius, &stencil))) return rc;
    const sph::ShellK sk = shell_consts(*cfg, radius);
    const bool fluidOnly = (cfg->flags & SPH_SHELL_FLUID_ONLY) != 0;
    const sph::HostGrid grid(k, particles, n);
    const std::vector<uint32_t>& order = grid.order;
    const std::vector<uint32_t>& slotOf = grid.slotOf;
    const size_t rows = query ? m : n;
    std::vector<sph::ShellRow> res(rows);
    SphShellInfo info{};
    info.rows = rows; info.radius = radius; info.stencil = stencil; info.kind = query ? 2 : 1; info.flags = cfg->flags;
    for (size_t r = 0; r < rows; ++r) {                                             // pass 1
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        sph::shell_zero(res[r]);
        if (sums4) sums4[4 * r] = sums4[4 * r + 1] = sums4[4 * r + 2] = sums4[4 * r + 3] = 0.0f;
        bool walk = sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2]);
        if (!query && fluidOnly && particles[r].isGhost != 0) walk = false;
        if (!walk) continue;
        sph::ShellAcc a;
        sph::shell_reset(a);
        grid.gather(stencil, x, sk.R2, particles, fluidOnly, query ? sph::HostGrid::kNoSlot : slotOf[r],
                    [&](float dx, float dy, float dz, float r2) { sph::shell_add(a, dx, dy, dz, r2, sk.R2); });
        sph::shell_finish(a, sk, res[r]);
        if (sums4) { sums4[4 * r] = a.Sx; sums4[4 * r + 1] = a.Sy; sums4[4 * r + 2] = a.Sz; sums4[4 * r + 3] = a.W; }
        if (res[r].flags & sph::kShellIsolated) info.numIsolated += 1u;
        info.maxCount = std::max(info.maxCount, res[r].count);
    }
    for (size_t r = 0; r < rows && !query; ++r) {                                   // pass 2: shell targets, shell candidates
        if (!(res[r].flags & sph::kShellMember)) continue;
        const float* x = particles[r].pos;
        const float* nrm = res[r].normal;
        long long crest = 0ll;
        grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
            for (uint32_t j = qs; j < qe; ++j) {
                const uint32_t o = order[j];
                if (!(res[o].flags & sph::kShellMember) || j == slotOf[r]) continue;
                const float* y = particles[o].pos;
                float dx, dy, dz, r2;
                if (!sph::neighbor_offset(x[0], x[1], x[2], y[0], y[1], y[2], sk.R2, dx, dy, dz, r2)) continue;
                crest += sph::shell_crest_term(nrm[0], nrm[1], nrm[2], res[o].normal[0], res[o].normal[1], res[o].normal[2], dx, dy, dz, r2, sk.R);
            }
        });
        res[r].crest = sph::shell_crest_value(crest);
    }
    for (size_t r = 0; r < rows; ++r) {
        if (!(res[r].flags & sph::kShellMember)) continue;
        if (ids) ids[info.numShell] = (int32_t)r;
        info.numShell += 1u;
    }
    if (rowsOut && rows) memcpy(rowsOut, res.data(), rows * sizeof(SphShell));
    *out = info;
    return SPH_OK;
}

// ---- ray casts (sph_rays.h) ------------------------------------------------------------------------
static_assert(sizeof(SphRayHit) == 32 && sizeof(SphRaysInfo) == 32, "SphRayHit and SphRaysInfo must be 32 bytes");
static_assert(SPH_RAYS_FLUID_ONLY == sph::kRaysFluidOnly && SPH_RAYS_ANY_HIT == sph::kRaysAnyHit, "sph_rays.h mirrors SPH_RAYS_*");

static int rays_check(float radius, float cellSize, int flags, size_t m) {
    if (flags & ~(SPH_RAYS_FLUID_ONLY | SPH_RAYS_ANY_HIT)) return fail(SPH_ERR_ARG, "unknown ray flags %d", flags);
    if (!std::isfinite(radius) || !(radius > 0.0f) || !(radius <= 0.5f * cellSize))
        return fail(SPH_ERR_ARG, "radius %g is not finite, not > 0 or above half a cell (%g)", (double)radius, (double)(0.5f * cellSize));
    if (m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu rays (at most 2^31 - 1)", m);
    return SPH_OK;
}
static int spans_check(float radius, float cellSize, int flags, size_t m) {
    if (flags & SPH_RAYS_ANY_HIT) return fail(SPH_ERR_ARG, "SPH_RAYS_ANY_HIT has no meaning for spans");
    return rays_check(radius, cellSize, flags, m);
}
static sph::RayK rays_consts(float radius, int flags, uint32_t idBase, size_t n) {
    sph::RayK rk;
    rk.r2 = radius * radius; rk.invr = 1.0f / radius; rk.flags = flags; rk.idBase = idBase; rk.n = (uint32_t)n;
    return rk;
}

// SPH_OPT_RAYS_VARIANT 1, for casts and spans: the scratch of the counting sort of m rays by their cell of entry, and its launches
// (d_rayOrder then holds the order).
static int rays_order_grow(SphEngine* e, size_t m, const SphGridInfo& g) {
    const size_t bins = (size_t)g.numCells + 1;
    int rc;
    if ((rc = e->d_rayBin.grow(e, m)) || (rc = e->d_rayOrder.grow(e, m)) || (rc = e->d_rayCount.grow(e, bins)) || (rc = e->d_rayStart.grow(e, bins + 1)) ||
        (rc = e->d_rayBlockSums.grow(e, (size_t)blocks_for(bins, kScanTile) + 1))) return rc;
    return SPH_OK;
}
static int rays_order_launch(SphEngine* e, const SimK& k, const float4* rays, size_t m) {
    using namespace sph;
    HIP_TRY(hipMemsetAsync(e->d_rayCount.p, 0, ((size_t)k.numCells + 1) * sizeof(uint32_t), e->stream));
    Timed t(e, SPH_K_OTHER);
    hipLaunchKernelGGL(k_rays_bin, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, rays, m, e->d_rayBin.p, e->d_rayCount.p);
    launch_cell_scan(e, e->d_rayCount.p, e->d_rayBlockSums.p, e->d_rayStart.p, k.numCells + 1, (uint32_t)m);
    hipLaunchKernelGGL(k_rays_order, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, (const uint2*)e->d_rayBin.p, (const uint32_t*)e->d_rayStart.p, m, e->d_rayOrder.p);
    return SPH_OK;
}

int sph_rays_cast_device(SphEngine* e, const float* devRays8, size_t m, float radius, int flags, SphRaysInfo* out) {
    using namespace sph;
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || (m && !devRays8)) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    SphGridInfo g;
    int rc;
    if ((rc = query_grid(e, g)) || (rc = rays_check(radius, g.cellSize, flags, m))) return rc;
    e->raysValid = false;                                                           // (the hits held so far end here)
    if ((rc = e->d_rayHits.grow(e, 2 * m)) || (rc = e->d_rayStats.grow(e, 2))) return rc;
    const bool ordered = e->optRaysVariant == 1 && m && e->n;
    if (ordered && (rc = rays_order_grow(e, m, g))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const RayK rk = rays_consts(radius, flags, e->idBase, e->n);
    const float4* rays = reinterpret_cast<const float4*>(devRays8);
    unsigned long long host[2] = {0ull, 0ull};
    if (m) {
        HIP_TRY(hipMemsetAsync(e->d_rayStats.p, 0, 2 * sizeof(unsigned long long), e->stream));
        if (ordered && (rc = rays_order_launch(e, k, rays, m))) return rc;
        {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_rays, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, rk, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                               (const float4*)e->d_sOwn, rays, ordered ? (const uint32_t*)e->d_rayOrder.p : (const uint32_t*)nullptr, m, e->d_rayHits.p, e->d_rayStats.p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, e->d_rayStats.p, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    SphRaysInfo info{};
    info.rays = m; info.hits = host[0]; info.voidRays = host[1]; info.radius = radius; info.flags = flags;
    e->raysInfo = info;
    e->raysValid = true;
    *out = info;
    return SPH_OK;
}

int sph_rays_cast(SphEngine* e, const float* rays8, size_t m, float radius, int flags, SphRaysInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || (m && !rays8)) return fail(SPH_ERR_ARG, "null argument");
    SphGridInfo g;
    int rc;
    if ((rc = query_grid(e, g)) || (rc = rays_check(radius, g.cellSize, flags, m))) return rc;   // (nothing is staged for a call that will be refused)
    if (m && (rc = e->d_rayIn.grow(e, 2 * m))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(e->d_rayIn.p, rays8, m * 2 * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    return sph_rays_cast_device(e, reinterpret_cast<const float*>(e->d_rayIn.p), m, radius, flags, out);
}

int sph_rays_info(const SphEngine* e, SphRaysInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->raysValid) return fail(SPH_ERR_STATE, "the engine holds no ray hits");
    *out = e->raysInfo;
    return SPH_OK;
}

int sph_rays_device(SphEngine* e, const SphRayHit** hits) {
    if (!e || !hits) return fail(SPH_ERR_ARG, "null argument");
    if (!e->raysValid) return fail(SPH_ERR_STATE, "the engine holds no ray hits");
    *hits = reinterpret_cast<const SphRayHit*>(e->d_rayHits.p);
    return SPH_OK;
}

int sph_rays_download(SphEngine* e, SphRayHit* hits) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->raysValid) return fail(SPH_ERR_STATE, "the engine holds no ray hits");
    const size_t m = (size_t)e->raysInfo.rays;
    if (m && !hits) return fail(SPH_ERR_ARG, "null argument");
    if (m) HIP_TRY(hipMemcpyAsync(hits, e->d_rayHits.p, m * sizeof(SphRayHit), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// What the host twins of casts and spans begin with: the checks (check: rays_check or spans_check), the grid's constants and who takes part.
static int rays_host_setup(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                           int (*check)(float, float, int, size_t), SimK& k, sph::RayK& rk, std::vector<uint8_t>& takesPart) {
    if (!params || (n && !particles) || (m && !rays8)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = check(radius, g.cellSize, flags, m))) return rc;
    rk = rays_consts(radius, flags, 0u, n);
    const bool fluidOnly = (flags & SPH_RAYS_FLUID_ONLY) != 0;
    takesPart.resize(n);
    for (size_t j = 0; j < n; ++j)
        takesPart[j] = !(fluidOnly && particles[j].isGhost != 0) && sph::ray_in_grid(k, particles[j].pos[0], particles[j].pos[1], particles[j].pos[2]);
    return SPH_OK;
}

// The definition: every ray against every participating record, no grid.  walk: sph_rays_walk_host, the device's ray_walk over the grid
// as the counting sort leaves it.
static int rays_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                     SphRayHit* hits, SphRaysInfo* out, bool walk);
int sph_rays_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                  SphRayHit* hits, SphRaysInfo* out) {
    return rays_host(particles, n, params, rays8, m, radius, flags, hits, out, false);
}
int sph_rays_walk_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                       SphRayHit* hits, SphRaysInfo* out) {
    return rays_host(particles, n, params, rays8, m, radius, flags, hits, out, true);
}
static int rays_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                     SphRayHit* hits, SphRaysInfo* out, bool walk) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    sph::RayK rk;
    std::vector<uint8_t> takesPart;
    int rc;
    if ((rc = rays_host_setup(particles, n, params, rays8, m, radius, flags, rays_check, k, rk, takesPart))) return rc;
    // for the walk: the grid of the records, and their positions in slot order
    const sph::HostGrid grid(k, particles, walk ? n : 0);
    const std::vector<uint32_t>& order = grid.order;
    std::vector<float4> spos(order.size());
    for (size_t j = 0; j < order.size(); ++j) spos[j] = make_float4(particles[order[j]].pos[0], particles[order[j]].pos[1], particles[order[j]].pos[2], 0.0f);
    auto rows = [&](int cx, int cy, int cz, auto&& f) { grid.rows(1, cx, cy, cz, f); };
    SphRaysInfo info{};
    info.rays = m; info.radius = radius; info.flags = flags;
    for (size_t i = 0; i < m; ++i) {
        sph::Ray R;
        unsigned long long best = sph::kRayNoKey;
        if (!sph::ray_setup(rays8 + 8 * i, R)) {
            info.voidRays += 1;
        } else if (walk) {
            uint32_t slot = 0u;
            best = sph::ray_walk(k, rk, R, rows, [&](uint32_t j) { return spos[j]; }, [&](uint32_t j) { return order[j]; },
                                 [&](uint32_t j) { return particles[order[j]].isGhost != 0; }, slot);
        } else {
            for (size_t j = 0; j < n; ++j) {
                float t;
                if (!takesPart[j] || !sph::ray_hit(R, rk.r2, particles[j].pos[0], particles[j].pos[1], particles[j].pos[2], t)) continue;
                best = std::min(best, sph::ray_key(t, (uint32_t)j));
            }
        }
        if (best != sph::kRayNoKey) info.hits += 1;
        if (hits) {
            const float* x = best != sph::kRayNoKey ? particles[(size_t)(best & 0xffffffffull)].pos : nullptr;
            float o8[8];
            sph::ray_write(R, rk, best, x ? x[0] : 0.0f, x ? x[1] : 0.0f, x ? x[2] : 0.0f, o8);
            memcpy(&hits[i], o8, sizeof(o8));
        }
    }
    *out = info;
    return SPH_OK;
}

// ---- ray spans (sph_rays.h "spans"): state of their own beside the hits; the staged rays and the ordering scratch are shared -----
static_assert(sizeof(SphRaySpan) == 32 && sizeof(SphRaySpansInfo) == 48, "SphRaySpan must be 32 bytes, SphRaySpansInfo 48");

int sph_rays_span_device(SphEngine* e, const float* devRays8, size_t m, float radius, int flags, SphRaySpansInfo* out) {
    using namespace sph;
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || (m && !devRays8)) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    SphGridInfo g;
    int rc;
    if ((rc = query_grid(e, g)) || (rc = spans_check(radius, g.cellSize, flags, m))) return rc;
    e->spansValid = false;                                                          // (the spans held so far end here)
    if ((rc = e->d_spanRows.grow(e, 2 * m)) || (rc = e->d_spanStats.grow(e, 4))) return rc;
    const bool ordered = e->optRaysVariant == 1 && m && e->n;
    if (ordered && (rc = rays_order_grow(e, m, g))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const RayK rk = rays_consts(radius, flags, e->idBase, e->n);
    const float4* rays = reinterpret_cast<const float4*>(devRays8);
    unsigned long long host[4] = {0ull, 0ull, 0ull, 0ull};
    if (m) {
        HIP_TRY(hipMemsetAsync(e->d_spanStats.p, 0, sizeof(host), e->stream));
        if (ordered && (rc = rays_order_launch(e, k, rays, m))) return rc;
        {
            Timed t(e, SPH_K_OTHER);
            auto kern = e->optRaySpansVariant == 1 ? k_ray_spans<true> : k_ray_spans<false>;
            hipLaunchKernelGGL(kern, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, rk, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                               (const float4*)e->d_sOwn, rays, ordered ? (const uint32_t*)e->d_rayOrder.p : (const uint32_t*)nullptr, m, e->d_spanRows.p, e->d_spanStats.p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, e->d_spanStats.p, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    SphRaySpansInfo info{};
    info.rays = m; info.crossed = host[0]; info.voidRays = host[1]; info.total = host[2]; info.maxCount = (uint32_t)host[3]; info.radius = radius; info.flags = flags;
    e->spansInfo = info;
    e->spansValid = true;
    *out = info;
    return SPH_OK;
}

int sph_rays_span(SphEngine* e, const float* rays8, size_t m, float radius, int flags, SphRaySpansInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out || (m && !rays8)) return fail(SPH_ERR_ARG, "null argument");
    SphGridInfo g;
    int rc;
    if ((rc = query_grid(e, g)) || (rc = spans_check(radius, g.cellSize, flags, m))) return rc;  // (nothing is staged for a call that will be refused)
    if (m && (rc = e->d_rayIn.grow(e, 2 * m))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(e->d_rayIn.p, rays8, m * 2 * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    return sph_rays_span_device(e, reinterpret_cast<const float*>(e->d_rayIn.p), m, radius, flags, out);
}

int sph_rays_span_info(const SphEngine* e, SphRaySpansInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->spansValid) return fail(SPH_ERR_STATE, "the engine holds no ray spans");
    *out = e->spansInfo;
    return SPH_OK;
}

int sph_rays_span_rows(SphEngine* e, const SphRaySpan** rows) {
    if (!e || !rows) return fail(SPH_ERR_ARG, "null argument");
    if (!e->spansValid) return fail(SPH_ERR_STATE, "the engine holds no ray spans");
    *rows = reinterpret_cast<const SphRaySpan*>(e->d_spanRows.p);
    return SPH_OK;
}

int sph_rays_span_download(SphEngine* e, SphRaySpan* rows) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->spansValid) return fail(SPH_ERR_STATE, "the engine holds no ray spans");
    const size_t m = (size_t)e->spansInfo.rays;
    if (m && !rows) return fail(SPH_ERR_ARG, "null argument");
    if (m) HIP_TRY(hipMemcpyAsync(rows, e->d_spanRows.p, m * sizeof(SphRaySpan), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// The definition (walk < 0): every ray against every participating record, no grid.  walk 0 / 1: ray_span_walk, layer / block, over
// the grid as the counting sort leaves it.
static int spans_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                      SphRaySpan* rowsOut, SphRaySpansInfo* out, int walk) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    sph::RayK rk;
    std::vector<uint8_t> takesPart;
    int rc;
    if ((rc = rays_host_setup(particles, n, params, rays8, m, radius, flags, spans_check, k, rk, takesPart))) return rc;
    const sph::HostGrid grid(k, particles, walk >= 0 ? n : 0);
    const std::vector<uint32_t>& order = grid.order;
    std::vector<float4> spos(order.size());
    for (size_t j = 0; j < order.size(); ++j) spos[j] = make_float4(particles[order[j]].pos[0], particles[order[j]].pos[1], particles[order[j]].pos[2], 0.0f);
    auto rows = [&](int x0, int x1, int y0, int y1, int z0, int z1, auto&& f) { sph::cell_box_rows(k, grid.start.data(), (uint32_t)order.size(), x0, x1, y0, y1, z0, z1, f); };
    auto pos = [&](uint32_t j) { return spos[j]; };
    auto id = [&](uint32_t j) { return order[j]; };
    auto ghost = [&](uint32_t j) { return particles[order[j]].isGhost != 0; };
    SphRaySpansInfo info{};
    info.rays = m; info.radius = radius; info.flags = flags;
    for (size_t i = 0; i < m; ++i) {
        sph::Ray R;
        sph::RaySpanAcc acc;
        const bool live = sph::ray_setup(rays8 + 8 * i, R);
        if (!live) {
            info.voidRays += 1;
        } else if (walk == 0) {
            sph::ray_span_walk<false>(k, rk, R, rows, pos, id, ghost, acc);
        } else if (walk == 1) {
            sph::ray_span_walk<true>(k, rk, R, rows, pos, id, ghost, acc);
        } else {
            for (size_t j = 0; j < n; ++j) {
                float tin, tout;
                uint32_t q;
                if (!takesPart[j] || !sph::ray_span(R, rk.r2, particles[j].pos[0], particles[j].pos[1], particles[j].pos[2], tin, tout, q)) continue;
                sph::ray_span_add(acc, tin, tout, q, (uint32_t)j);
            }
        }
        if (acc.count) info.crossed += 1;
        info.total += acc.count;
        info.maxCount = std::max(info.maxCount, acc.count);
        if (rowsOut) {
            uint32_t o8[8];
            sph::ray_span_write(acc, !live, o8);
            memcpy(&rowsOut[i], o8, sizeof(o8));
        }
    }
    *out = info;
    return SPH_OK;
}
int sph_rays_span_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                       SphRaySpan* rows, SphRaySpansInfo* out) {
    return spans_host(particles, n, params, rays8, m, radius, flags, rows, out, -1);
}
int sph_rays_span_walk_host(const SphParticle* particles, size_t n, const SphParams* params, const float* rays8, size_t m, float radius, int flags,
                            int variant, SphRaySpan* rows, SphRaySpansInfo* out) {
    if (variant < 0 || variant > 1) return fail(SPH_ERR_ARG, "span walk variant %d (0 = layer walk, 1 = block walk)", variant);
    return spans_host(particles, n, params, rays8, m, radius, flags, rows, out, variant);
}

// ---- iso-surface meshes (sph_surface.h) ----------------------------------------------------------
static int surface_check_lattice(const float origin[3], const float spacing[3], const int dims[3], float iso) {
    if (!origin) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = check_lattice(dims, spacing, 2, nullptr))) return rc;
    if (!std::isfinite(iso)) return fail(SPH_ERR_ARG, "iso %g is not finite", (double)iso);
    return SPH_OK;
}

// Count, scan, one synchronisation for the totals, then the vertex and triangle kernels (arguments already checked).
static int surface_mesh(SphEngine* e, const float* vol, const float origin[3], const float spacing[3], const int dims[3], float iso, SphSurface* out) {
    using namespace sph;
    SurfK s;
    s.ox = origin[0]; s.oy = origin[1]; s.oz = origin[2];
    s.sx = spacing[0]; s.sy = spacing[1]; s.sz = spacing[2];
    s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2];
    s.npts = (long long)dims[0] * dims[1] * dims[2];
    s.iso = iso;
    s.nTiles = (int)((s.npts + kSurfTile - 1) / kSurfTile);
    int rc;
    if ((rc = e->d_surfCode.grow(e, (size_t)s.npts)) || (rc = e->d_surfVOff.grow(e, (size_t)s.npts)) ||
        (rc = e->d_surfTile.grow(e, (size_t)s.nTiles)) ||
        (rc = e->d_surfTileOff.grow(e, 2 * (size_t)s.nTiles + 2))) return rc;
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_surf_count, dim3(s.nTiles), dim3(kBlock), 0, e->stream, s, vol, e->d_surfCode.p, e->d_surfTile.p);
    }
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_surf_scan_tiles, dim3(1), dim3(kBlock), 0, e->stream, (const uint2*)e->d_surfTile.p, e->d_surfTileOff.p, s.nTiles);
    }
    HIP_TRY(hipGetLastError());
    unsigned long long tot[2] = {0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(tot, e->d_surfTileOff.p + 2 * (size_t)s.nTiles, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (tot[0] > 0xFFFFFFFFull || tot[1] > 0xFFFFFFFFull)
        return fail(SPH_ERR_CAPACITY, "surface of %llu vertices and %llu triangles exceeds 2^32 - 1", tot[0], tot[1]);
    if ((rc = e->d_surfVerts.grow(e, (size_t)tot[0])) ||
        (rc = e->d_surfTris.grow(e, 3 * (size_t)tot[1]))) return rc;
    if (tot[0]) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_surf_vertices, dim3(s.nTiles), dim3(kBlock), 0, e->stream, s, vol, (const uint16_t*)e->d_surfCode.p,
                           (const unsigned long long*)e->d_surfTileOff.p, e->d_surfVOff.p, e->d_surfVerts.p);
    }
    if (tot[1]) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_surf_triangles, dim3(s.nTiles), dim3(kBlock), 0, e->stream, s, (const uint16_t*)e->d_surfCode.p,
                           (const uint32_t*)e->d_surfVOff.p, (const unsigned long long*)e->d_surfTileOff.p, e->d_surfTris.p);
    }
    HIP_TRY(hipGetLastError());
    e->surfNumV = (uint32_t)tot[0];
    e->surfNumT = (uint32_t)tot[1];
    e->surfValid = true;
    out->numVertices = e->surfNumV;
    out->numTriangles = e->surfNumT;
    out->vertices = e->surfNumV ? reinterpret_cast<const SphSurfaceVertex*>(e->d_surfVerts.p) : nullptr;
    out->triangles = e->surfNumT ? e->d_surfTris.p : nullptr;
    return SPH_OK;
}

int sph_extract_surface_volume(SphEngine* e, const float* devValues, const float origin[3], const float spacing[3], const int dims[3], float iso,
                               SphSurface* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    e->surfValid = false;                                             // (any failure below leaves no surface: sph_abi.h)
    if (!devValues || !out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = surface_check_lattice(origin, spacing, dims, iso))) return rc;
    return surface_mesh(e, devValues, origin, spacing, dims, iso, out);
}

int sph_extract_surface(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int field, float iso, SphSurface* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    e->surfValid = false;
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = surface_check_lattice(origin, spacing, dims, iso))) return rc;
    if (field < SPH_FIELD_DENSITY || field > SPH_FIELD_SPEED) return fail(SPH_ERR_ARG, "field %d is not a scalar field", field);
    if ((rc = query_refused(e))) return rc;
    const size_t npts = (size_t)dims[0] * dims[1] * dims[2];
    if ((rc = e->d_surfVol.grow(e, npts))) return rc;
    if ((rc = sph_sample_lattice(e, origin, spacing, dims, field, e->d_surfVol.p))) return rc;
    return surface_mesh(e, e->d_surfVol.p, origin, spacing, dims, iso, out);
}

int sph_surface_download(SphEngine* e, SphSurfaceVertex* vertices, size_t vertexCap, uint32_t* triangles3, size_t triangleCap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->surfValid) return fail(SPH_ERR_STATE, "no surface: call sph_extract_surface or sph_extract_surface_volume first");
    if (vertexCap < e->surfNumV || triangleCap < e->surfNumT)
        return fail(SPH_ERR_CAPACITY, "surface has %u vertices and %u triangles (capacities %zu, %zu)", e->surfNumV, e->surfNumT, vertexCap, triangleCap);
    if ((e->surfNumV && !vertices) || (e->surfNumT && !triangles3)) return fail(SPH_ERR_ARG, "null argument");
    if (e->surfNumV) HIP_TRY(hipMemcpyAsync(vertices, e->d_surfVerts.p, (size_t)e->surfNumV * sizeof(SphSurfaceVertex), hipMemcpyDeviceToHost, e->stream));
    if (e->surfNumT) HIP_TRY(hipMemcpyAsync(triangles3, e->d_surfTris.p, (size_t)e->surfNumT * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// ---- anisotropic kernels (sph_aniso.h; behind the surface section: sph_aniso_surface ends in its mesher) ------
static_assert(sizeof(SphAniso) == 64 && sizeof(SphAnisoConfig) == 32 && sizeof(SphAnisoInfo) == 56, "SphAniso is 64 bytes, SphAnisoConfig 32, SphAnisoInfo 56");
static_assert(sizeof(sph::AnisoRow) == sizeof(SphAniso) && offsetof(sph::AnisoRow, count) == offsetof(SphAniso, count) &&
              offsetof(sph::AnisoRow, flags) == offsetof(SphAniso, flags) && offsetof(sph::AnisoRow, reach) == offsetof(SphAniso, reach) &&
              offsetof(sph::AnisoRow, amplitude) == offsetof(SphAniso, amplitude), "sph_aniso.h mirrors SphAniso");
static_assert(SPH_ANISO_FLUID_ONLY == sph::kAnisoFluidOnly && SPH_ANISO_VALID == sph::kAnisoValid && SPH_ANISO_SPARSE == sph::kAnisoSparse &&
              SPH_ANISO_CLAMPED == sph::kAnisoClamped, "sph_aniso.h mirrors SPH_ANISO_*");

void sph_aniso_default(SphAnisoConfig* cfg) {
    if (!cfg) return;
    cfg->radius = 0.0f; cfg->support = 0.0f; cfg->smoothing = 0.9f; cfg->maxRatio = 4.0f; cfg->maxStretch = 1.5f; cfg->sparseScale = 0.5f;
    cfg->minCount = 25u; cfg->flags = 0;
}

// The config as an argument: the constants of a build (radius and support in force), the stencil half-width through *stencil.
static int aniso_check(const SphAnisoConfig& cfg, float h, float cellSize, sph::AnisoK* ak, float* radius, int* stencil) {
    if (cfg.flags & ~SPH_ANISO_FLUID_ONLY) return fail(SPH_ERR_ARG, "unknown anisotropy flags %d", cfg.flags);
    if (!std::isfinite(cfg.support)) return fail(SPH_ERR_ARG, "support %g is not finite", (double)cfg.support);
    if (!(cfg.smoothing >= 0.0f && cfg.smoothing <= 1.0f)) return fail(SPH_ERR_ARG, "smoothing %g is not in [0, 1]", (double)cfg.smoothing);
    if (!std::isfinite(cfg.maxRatio) || !(cfg.maxRatio >= 1.0f)) return fail(SPH_ERR_ARG, "maxRatio %g is not finite or < 1", (double)cfg.maxRatio);
    if (!std::isfinite(cfg.maxStretch) || !(cfg.maxStretch > 0.0f)) return fail(SPH_ERR_ARG, "maxStretch %g is not finite or <= 0", (double)cfg.maxStretch);
    if (!std::isfinite(cfg.sparseScale) || !(cfg.sparseScale > 0.0f)) return fail(SPH_ERR_ARG, "sparseScale %g is not finite or <= 0", (double)cfg.sparseScale);
    *radius = cfg.radius <= 0.0f ? 2.0f * h : cfg.radius;
    int rc;
    if ((rc = radius_stencil(*radius, cellSize, stencil))) return rc;
    ak->R2 = *radius * *radius;
    ak->scale = 11.0f / ak->R2;
    ak->support = cfg.support <= 0.0f ? h : cfg.support;
    ak->lambda = cfg.smoothing; ak->maxRatio = cfg.maxRatio; ak->maxStretch = cfg.maxStretch; ak->sparseScale = cfg.sparseScale;
    ak->minCount = cfg.minCount;
    return SPH_OK;
}
// A lattice of nodes as an argument of the anisotropic field: check_lattice with dimensions >= 0 (a 0 is an empty lattice: *total 0).
static int aniso_check_lattice(const float origin[3], const float spacing[3], const int dims[3], long long* total) {
    if (!origin) return fail(SPH_ERR_ARG, "null argument");
    return check_lattice(dims, spacing, 0, total);
}
static void aniso_fill_info(SphAnisoInfo& info, size_t rows, float radius, float support, int stencil, float cellSize, int flags) {
    info.rows = rows; info.radius = radius; info.support = support; info.stencil = stencil; info.kind = 1; info.flags = flags;
    info.reachStencil = sph::neighbor_stencil(info.maxReach, cellSize);
}
// The field needs every ellipsoid inside the widest stencil.
static int aniso_check_reach(const SphAnisoInfo& info, float cellSize) {
    if (!(info.maxReach <= 3.0f * cellSize))
        return fail(SPH_ERR_ARG, "maxReach %g is above three cells (%g): lower support, maxStretch or smoothing", (double)info.maxReach, (double)(3.0f * cellSize));
    return SPH_OK;
}

// Grid of the current state, ids, the gather, one synchronisation for the four words of the reduction.  *kOut / *cellSize: the grid it ran on.
static int aniso_run(SphEngine* e, const SphAnisoConfig& cfg, SphAnisoInfo* out, SimK* kOut, float* cellSize) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    AnisoK ak;
    int rc, stencil = 0;
    float radius = 0.0f;
    if ((rc = query_grid(e, g)) || (rc = aniso_check(cfg, e->params.param_h, g.cellSize, &ak, &radius, &stencil))) return rc;
    const size_t n = e->n;
    e->anisoInfo = SphAnisoInfo{};                                                  // (the rows held so far end here)
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_anRows.grow(e, n)) || (rc = e->d_anSlots.grow(e, 3 * n)) || (rc = e->d_anStats.grow(e, 4))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, radius, stencil, cfg.flags, e->n);
    unsigned long long stats[4] = {0ull, 0ull, 0ull, 0ull};
    if (n) {
        HIP_TRY(hipMemsetAsync(e->d_anStats.p, 0, sizeof(stats), e->stream));
        slot_ids_fill(e);
        {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_aniso_gather, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, k, nb, ak, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                               (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn, n, e->d_anRows.p, e->d_anSlots.p, e->d_anStats.p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(stats, e->d_anStats.p, sizeof(stats), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    SphAnisoInfo info{};
    info.numSparse = stats[0]; info.numClamped = stats[1]; info.maxCount = (uint32_t)stats[2];
    const uint32_t reachBits = (uint32_t)stats[3];
    memcpy(&info.maxReach, &reachBits, 4);
    aniso_fill_info(info, n, radius, ak.support, stencil, g.cellSize, cfg.flags);
    e->anisoInfo = info;
    *out = info;
    if (kOut) *kOut = k;
    if (cellSize) *cellSize = g.cellSize;
    return SPH_OK;
}

int sph_aniso_build(SphEngine* e, const SphAnisoConfig* cfg, SphAnisoInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !out) return fail(SPH_ERR_ARG, "null argument");
    return aniso_run(e, *cfg, out, nullptr, nullptr);
}

int sph_aniso_info(const SphEngine* e, SphAnisoInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->anisoInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no anisotropy rows");
    *out = e->anisoInfo;
    return SPH_OK;
}

int sph_aniso_device(SphEngine* e, const SphAniso** rows) {
    if (!e || !rows) return fail(SPH_ERR_ARG, "null argument");
    if (!e->anisoInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no anisotropy rows");
    *rows = reinterpret_cast<const SphAniso*>(e->d_anRows.p);
    return SPH_OK;
}

int sph_aniso_download(SphEngine* e, SphAniso* rows) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->anisoInfo.kind) return fail(SPH_ERR_STATE, "the engine holds no anisotropy rows");
    const size_t r = (size_t)e->anisoInfo.rows;
    if (rows && r) HIP_TRY(hipMemcpyAsync(rows, e->d_anRows.p, r * sizeof(SphAniso), hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// The rows, then the lattice kernel behind them (arguments already checked; total > 0 nodes or none).
static int aniso_lattice_run(SphEngine* e, const SphAnisoConfig& cfg, const float origin[3], const float spacing[3], const int dims[3], long long total,
                             float* devOut, SphAnisoInfo* out) {
    using namespace sph;
    SimK k;
    float cellSize = 0.0f;
    int rc;
    if ((rc = aniso_run(e, cfg, out, &k, &cellSize)) || (rc = aniso_check_reach(*out, cellSize))) return rc;
    if (!total) return SPH_OK;
    const LatticeK L = lattice_consts(origin, spacing, dims, kFieldFraction, 0);      // (field and stage are not read)
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_aniso_lattice, dim3((unsigned)std::min<long long>(L.nBricks, 1ll << 20)), dim3(kBlock), 0, e->stream, k, L, out->reachStencil,
                           (uint32_t)e->n, e->params.param_mass, (const float4*)e->d_anSlots.p, (const uint32_t*)e->d_cellStart, devOut);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aniso_lattice(SphEngine* e, const SphAnisoConfig* cfg, const float origin[3], const float spacing[3], const int dims[3], float* devOut, SphAnisoInfo* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !out) return fail(SPH_ERR_ARG, "null argument");
    long long total = 0;
    int rc;
    if ((rc = aniso_check_lattice(origin, spacing, dims, &total))) return rc;
    if (total && !devOut) return fail(SPH_ERR_ARG, "null argument");
    return aniso_lattice_run(e, *cfg, origin, spacing, dims, total, devOut, out);
}

int sph_aniso_surface(SphEngine* e, const SphAnisoConfig* cfg, const float origin[3], const float spacing[3], const int dims[3], float iso, SphSurface* out,
                      SphAnisoInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    e->surfValid = false;                                             // (any failure below leaves no surface: sph_abi.h)
    if (!cfg || !out || !info) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = surface_check_lattice(origin, spacing, dims, iso)) || (rc = query_refused(e))) return rc;
    const size_t npts = (size_t)dims[0] * dims[1] * dims[2];
    if ((rc = e->d_surfVol.grow(e, npts))) return rc;
    if ((rc = aniso_lattice_run(e, *cfg, origin, spacing, dims, (long long)npts, e->d_surfVol.p, info))) return rc;
    return surface_mesh(e, e->d_surfVol.p, origin, spacing, dims, iso, out);
}

// The rows and the slot records (by sorted slot of `grid`) of host records: what both twins start from.
static void aniso_rows_host(const SphParticle* particles, size_t n, const sph::HostGrid& grid, int stencil, const sph::AnisoK& ak, bool fluidOnly,
                            std::vector<sph::AnisoRow>& res, std::vector<sph::AnisoSlot>& slots, SphAnisoInfo& info) {
    res.resize(n);
    slots.resize(n);
    for (size_t r = 0; r < n; ++r) {
        const float* x = particles[r].pos;
        sph::AnisoSlot& slot = slots[grid.slotOf[r]];
        sph::aniso_zero(res[r], slot);
        bool walk = sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2]);
        if (fluidOnly && particles[r].isGhost != 0) walk = false;
        if (!walk) continue;
        sph::AnisoAcc a;
        sph::aniso_reset(a);
        grid.gather(stencil, x, ak.R2, particles, fluidOnly, sph::HostGrid::kNoSlot,
                    [&](float dx, float dy, float dz, float r2) { sph::aniso_add(a, dx, dy, dz, r2, ak.R2); });
        const float invRho = particles[r].density > 0.0f ? 1.0f / particles[r].density : 0.0f;
        if (a.cnt) sph::aniso_finish(a, ak, x[0], x[1], x[2], invRho, res[r], slot);
        if (res[r].flags & sph::kAnisoSparse) info.numSparse += 1u;
        if (res[r].flags & sph::kAnisoClamped) info.numClamped += 1u;
        info.maxCount = std::max(info.maxCount, res[r].count);
        if (res[r].reach > info.maxReach) info.maxReach = res[r].reach;
    }
}

// What both twins open with: the params, the grid they give, the config; then the rows.
static int aniso_host_open(const SphParticle* particles, size_t n, const SphParams* params, const SphAnisoConfig* cfg, SimK& k, SphGridInfo& g,
                           sph::AnisoK& ak, float* radius, int* stencil) {
    if (!params || !cfg || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    sph::compute_grid_extents(*params, g);
    sph::make_simk(*params, g, params->param_timeStep, k);
    return aniso_check(*cfg, params->param_h, g.cellSize, &ak, radius, stencil);
}

int sph_aniso_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAnisoConfig* cfg, SphAniso* rowsOut, SphAnisoInfo* out) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    SphGridInfo g;
    sph::AnisoK ak;
    int rc, stencil = 0;
    float radius = 0.0f;
    if ((rc = aniso_host_open(particles, n, params, cfg, k, g, ak, &radius, &stencil))) return rc;
    const sph::HostGrid grid(k, particles, n);
    std::vector<sph::AnisoRow> res;
    std::vector<sph::AnisoSlot> slots;
    SphAnisoInfo info{};
    aniso_rows_host(particles, n, grid, stencil, ak, (cfg->flags & SPH_ANISO_FLUID_ONLY) != 0, res, slots, info);
    aniso_fill_info(info, n, radius, ak.support, stencil, g.cellSize, cfg->flags);
    if (rowsOut && n) memcpy(rowsOut, res.data(), n * sizeof(SphAniso));
    *out = info;
    return SPH_OK;
}

int sph_aniso_lattice_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAnisoConfig* cfg, const float origin[3],
                           const float spacing[3], const int dims[3], float* values, SphAnisoInfo* out) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    long long total = 0;
    int rc, stencil = 0;
    if ((rc = aniso_check_lattice(origin, spacing, dims, &total))) return rc;
    if (total && !values) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    SphGridInfo g;
    sph::AnisoK ak;
    float radius = 0.0f;
    if ((rc = aniso_host_open(particles, n, params, cfg, k, g, ak, &radius, &stencil))) return rc;
    const sph::HostGrid grid(k, particles, n);
    std::vector<sph::AnisoRow> res;
    std::vector<sph::AnisoSlot> slots;
    SphAnisoInfo info{};
    aniso_rows_host(particles, n, grid, stencil, ak, (cfg->flags & SPH_ANISO_FLUID_ONLY) != 0, res, slots, info);
    aniso_fill_info(info, n, radius, ak.support, stencil, g.cellSize, cfg->flags);
    *out = info;
    if ((rc = aniso_check_reach(info, g.cellSize))) return rc;
    for (long long p = 0; p < total; ++p) {
        const int i = (int)(p % dims[0]), j = (int)((p / dims[0]) % dims[1]), l = (int)(p / ((long long)dims[0] * dims[1]));
        const float x[3] = {sph::aniso_coord(origin[0], i, spacing[0]), sph::aniso_coord(origin[1], j, spacing[1]), sph::aniso_coord(origin[2], l, spacing[2])};
        float acc = 0.0f;
        const bool finite = sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2]);
        if (finite) {
            grid.rows(info.reachStencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t q = qs; q < qe; ++q) {
                    const sph::AnisoSlot& s = slots[q];
                    float rx, ry, rz;
                    if (!sph::aniso_node_near(x[0], x[1], x[2], s.cx, s.cy, s.cz, s.rho2, rx, ry, rz)) continue;
                    acc = sph::aniso_node_term(rx, ry, rz, s.qxx, s.qyy, s.qzz, s.qxy, s.qxz, s.qyz, s.amp, acc);
                }
            });
        }
        values[p] = finite ? sph::aniso_node_value(params->param_mass, acc) : 0.0f;
    }
    return SPH_OK;
}

// ---- fused neighbourhood reductions of caller tensors (sph_aggregate.h) ---------------------------------
static_assert(sizeof(SphAggregateConfig) == 32 && sizeof(SphAggregateInfo) == 32, "SphAggregateConfig is 32 bytes, SphAggregateInfo 32");
static_assert(SPH_AGGREGATE_SELF == sph::kAggSelf && SPH_AGGREGATE_FLUID_ONLY == sph::kAggFluidOnly && SPH_AGGREGATE_DELTA == sph::kAggDelta &&
              SPH_AGGREGATE_MOMENTS == sph::kAggMoments && SPH_AGGREGATE_SUM == sph::kAggSum && SPH_AGGREGATE_MEAN == sph::kAggMean &&
              SPH_AGGREGATE_MAX == sph::kAggMax && SPH_AGGREGATE_MIN == sph::kAggMin && SPH_AGGREGATE_WEIGHT_ONE == sph::kAggWeightOne &&
              SPH_AGGREGATE_WEIGHT_POLY6 == sph::kAggWeightPoly6 && SPH_AGGREGATE_MAX_CHANNELS == sph::kAggMaxChannels, "sph_aggregate.h mirrors SPH_AGGREGATE_*");

void sph_aggregate_default(SphAggregateConfig* cfg) {
    if (!cfg) return;
    *cfg = SphAggregateConfig{};
    cfg->op = SPH_AGGREGATE_SUM;
    cfg->weight = SPH_AGGREGATE_WEIGHT_ONE;
    cfg->channels = 1;
}

// The config as an argument: the stencil half-width through *stencil.
static int aggregate_check(const SphAggregateConfig& c, float cellSize, bool query, int* stencil) {
    if (c.op < SPH_AGGREGATE_SUM || c.op > SPH_AGGREGATE_MIN) return fail(SPH_ERR_ARG, "unknown aggregate op %d", c.op);
    if (c.weight < SPH_AGGREGATE_WEIGHT_ONE || c.weight > SPH_AGGREGATE_WEIGHT_POLY6) return fail(SPH_ERR_ARG, "unknown aggregate weight %d", c.weight);
    if (c.flags & ~(SPH_AGGREGATE_SELF | SPH_AGGREGATE_FLUID_ONLY | SPH_AGGREGATE_DELTA | SPH_AGGREGATE_MOMENTS)) return fail(SPH_ERR_ARG, "unknown aggregate flags %d", c.flags);
    if (c.pad[0] || c.pad[1] || c.pad[2]) return fail(SPH_ERR_ARG, "the padding of SphAggregateConfig must be zero");
    if (c.channels < 1 || c.channels > SPH_AGGREGATE_MAX_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (1 .. %d)", c.channels, (int)SPH_AGGREGATE_MAX_CHANNELS);
    if ((c.flags & SPH_AGGREGATE_MOMENTS) && c.op != SPH_AGGREGATE_SUM) return fail(SPH_ERR_ARG, "SPH_AGGREGATE_MOMENTS goes with SPH_AGGREGATE_SUM only");
    if ((c.op == SPH_AGGREGATE_MAX || c.op == SPH_AGGREGATE_MIN) && c.weight != SPH_AGGREGATE_WEIGHT_ONE) return fail(SPH_ERR_ARG, "SPH_AGGREGATE_MAX / _MIN take the weight ONE");
    if (query && (c.flags & (SPH_AGGREGATE_SELF | SPH_AGGREGATE_DELTA))) return fail(SPH_ERR_ARG, "SPH_AGGREGATE_SELF / _DELTA apply to particle targets only");
    return radius_stencil(c.radius, cellSize, stencil);
}

static int aggregate_planes(const SphAggregateConfig& c) { return (c.flags & SPH_AGGREGATE_MOMENTS) ? 4 : 1; }

// Do [a, a + aBytes) and [b, b + bBytes) share an address?
static bool ranges_overlap(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return aBytes && bBytes && a0 < b0 + bBytes && b0 < a0 + aBytes;
}

// One launch of the instance the config and SPH_OPT_AGGREGATE_VARIANT select (arguments already checked).
static void aggregate_launch(SphEngine* e, bool query, const sph::SimK& k, const sph::NbK& nb, const sph::AggK& ag, int chunk, bool moments, const float4* devPoints,
                             size_t rows, const float* vals, float* devOut, uint32_t* devCount) {
    using namespace sph;
    using Kernel = void (*)(SimK, NbK, AggK, const float4*, const uint32_t*, const int32_t*, const float4*, const float4*, size_t, const float*, float*, uint32_t*);
    const bool extremum = ag.op == kAggMax || ag.op == kAggMin;
    auto pick = [&](auto ch) -> Kernel {
        constexpr int CH = decltype(ch)::value;
        if (extremum) return query ? (Kernel)k_aggregate<false, true, false, CH> : (Kernel)k_aggregate<true, true, false, CH>;
        if (moments) return query ? (Kernel)k_aggregate<false, false, true, CH> : (Kernel)k_aggregate<true, false, true, CH>;
        return query ? (Kernel)k_aggregate<false, false, false, CH> : (Kernel)k_aggregate<true, false, false, CH>;
    };
    const Kernel kernel = chunk == 4 ? pick(std::integral_constant<int, 4>{}) : chunk == 8 ? pick(std::integral_constant<int, 8>{}) : pick(std::integral_constant<int, 16>{});
    hipLaunchKernelGGL(kernel, dim3(blocks_for(rows)), dim3(kBlock), 0, e->stream, k, nb, ag, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                       (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn, devPoints, rows, vals, devOut, devCount);
}

// Grid of the current state, ids, the stage (default variant), the walk.  No synchronisation: nothing is read back.
static int aggregate_run(SphEngine* e, bool query, const SphAggregateConfig* cfg, const float4* devPoints, size_t m, const float* devValues, float* devOut,
                         uint32_t* devCount, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = aggregate_check(*cfg, g.cellSize, query, &stencil))) return rc;
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (rows > ((size_t)-1) / (planes * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, planes, C);
    const size_t outBytes = rows * planes * C * sizeof(float), valBytes = n * C * sizeof(float);
    if (ranges_overlap(devOut, outBytes, devValues, valBytes) || ranges_overlap(devCount, devCount ? rows * sizeof(uint32_t) : 0, devValues, valBytes))
        return fail(SPH_ERR_ARG, "the output overlaps the values");
    SphAggregateInfo info{};
    info.rows = rows; info.channels = cfg->channels; info.planes = (int32_t)planes; info.stencil = stencil; info.flags = cfg->flags; info.radius = cfg->radius;
    *out = info;
    if (!rows || !n) return SPH_OK;
    const int variant = e->optAggVariant;
    const bool byId = (variant & 1) != 0;
    const int chunkSel = (variant >> 1) & 3, chunk = chunkSel ? 2 << chunkSel : aggregate_chunk(cfg->channels);
    if ((rc = e->d_slotIds.grow(e, n)) || (!byId && (rc = e->d_aggStage.grow(e, n * C)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const float* vals = byId ? devValues : e->d_aggStage.p;
    const AggK ag{cfg->op, cfg->weight, cfg->channels, byId ? 1 : 0, (!(variant & 8) && C % 4 == 0 && (uintptr_t)vals % 16 == 0) ? 1 : 0};
    slot_ids_fill(e);
    if (!byId) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * C)), dim3(kBlock), 0, e->stream, (const int32_t*)e->d_slotIds.p, devValues, e->d_aggStage.p, (uint32_t)n, cfg->channels);
    }
    {
        Timed t(e, SPH_K_OTHER);
        aggregate_launch(e, query, k, nb, ag, chunk, planes == 4, devPoints, rows, vals, devOut, devCount);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info || (e->n && (!devValues || !devOut))) return fail(SPH_ERR_ARG, "null argument");
    return aggregate_run(e, false, cfg, nullptr, 0, devValues, devOut, devCount, info);
}

int sph_aggregate_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                        uint32_t* devCount, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info || (m && e->n && (!devPoints4 || !devValues || !devOut))) return fail(SPH_ERR_ARG, "null argument");
    if (m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    return aggregate_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devValues, devOut, devCount, info);
}

// Host memory in and out through engine scratch: the upload, the device call, the download, one synchronisation.
int sph_aggregate_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* values, float* out, uint32_t* count,
                         SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = aggregate_check(*cfg, g.cellSize, query, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, cells = rows * (size_t)aggregate_planes(*cfg) * C;
    const bool work = rows && n;
    if (work && (!values || !out)) return fail(SPH_ERR_ARG, "null argument");
    if (work && ((rc = e->d_aggIn.grow(e, n * C)) || (rc = e->d_aggOut.grow(e, cells)) || (rc = e->d_aggCnt.grow(e, rows)) ||
                 (query && (rc = e->d_sampleIn.grow(e, m))))) return rc;
    if (work) HIP_TRY(hipMemcpyAsync(e->d_aggIn.p, values, n * C * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (work && query) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = aggregate_run(e, query, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, e->d_aggIn.p, e->d_aggOut.p,
                            count ? e->d_aggCnt.p : nullptr, info))) return rc;
    if (work) HIP_TRY(hipMemcpyAsync(out, e->d_aggOut.p, cells * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (work && count) HIP_TRY(hipMemcpyAsync(count, e->d_aggCnt.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_aggregate_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                       const float* values, float* out, uint32_t* count) {
    if (!params || !cfg || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    int rc, stencil = 0;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, params->param_timeStep, k);
    if ((rc = aggregate_check(*cfg, g.cellSize, query, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (!rows || !n) return SPH_OK;
    if (!values || !out) return fail(SPH_ERR_ARG, "null argument");
    if (ranges_overlap(out, rows * planes * C * sizeof(float), values, n * C * sizeof(float)) ||
        ranges_overlap(count, count ? rows * sizeof(uint32_t) : 0, values, n * C * sizeof(float))) return fail(SPH_ERR_ARG, "the output overlaps the values");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const bool delta = !query && (cfg->flags & SPH_AGGREGATE_DELTA) != 0, moments = planes == 4;
    const bool extremum = cfg->op == SPH_AGGREGATE_MAX || cfg->op == SPH_AGGREGATE_MIN, isMax = cfg->op == SPH_AGGREGATE_MAX;
    const sph::HostGrid grid(k, particles, n);
    std::vector<float> acc(planes * C);
    std::vector<uint32_t> best(C);
    for (size_t r = 0; r < rows; ++r) {
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
        std::fill(acc.begin(), acc.end(), 0.0f);
        std::fill(best.begin(), best.end(), isMax ? sph::kAggLowest : sph::kAggHighest);
        float W = 0.0f;
        uint32_t cnt = 0u;
        const float* mine = values + (query ? 0 : r) * C;
        if (walk) {
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    const SphParticle& cand = particles[grid.order[j]];
                    float dx, dy, dz, r2;
                    if (!sph::aggregate_accept(!query && j == grid.slotOf[r], self, x[0], x[1], x[2], cand.pos[0], cand.pos[1], cand.pos[2], R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && cand.isGhost != 0) continue;
                    const float* v = values + (size_t)grid.order[j] * C;
                    const float w = sph::aggregate_weight(cfg->weight, R2, r2);
                    cnt += 1u;
                    W = W + w;
                    for (size_t c = 0; c < C; ++c) {
                        const float val = sph::aggregate_value(delta, v[c], mine[c]);
                        if (extremum) {
                            best[c] = sph::aggregate_extremum(isMax, best[c], val);
                            continue;
                        }
                        acc[c] = sph::aggregate_add(acc[c], w, val);
                        if (!moments) continue;
                        acc[C + c] = sph::aggregate_add_moment(acc[C + c], w, dx, val);
                        acc[2 * C + c] = sph::aggregate_add_moment(acc[2 * C + c], w, dy, val);
                        acc[3 * C + c] = sph::aggregate_add_moment(acc[3 * C + c], w, dz, val);
                    }
                }
            });
        }
        float* orow = out + r * planes * C;
        for (size_t c = 0; c < C; ++c) {
            if (extremum) { orow[c] = sph::agg_unordered(best[c]); continue; }
            orow[c] = cfg->op == SPH_AGGREGATE_MEAN ? sph::aggregate_mean(acc[c], W) : acc[c];
            for (size_t p = 1; p < planes; ++p) orow[p * C + c] = acc[p * C + c];
        }
        if (count) count[r] = cnt;
    }
    return SPH_OK;
}

// ---- the adjoint of the neighbourhood sums, extrema with their winners, routing through them (sph_aggregate.h) ----
// The forward's config plus the op the family takes: SUM for the adjoint, MAX / MIN for the winners and the routing.
static int adjoint_check(const SphAggregateConfig& c, float cellSize, bool query, bool extremum, int* stencil) {
    int rc;
    if ((rc = aggregate_check(c, cellSize, query, stencil))) return rc;
    if (!extremum && c.op != SPH_AGGREGATE_SUM) return fail(SPH_ERR_ARG, "the adjoint is that of SPH_AGGREGATE_SUM (op %d)", c.op);
    if (extremum && c.op != SPH_AGGREGATE_MAX && c.op != SPH_AGGREGATE_MIN) return fail(SPH_ERR_ARG, "winners are those of SPH_AGGREGATE_MAX / _MIN (op %d)", c.op);
    return SPH_OK;
}

// The counting sort of m query points by clamped cell into (cell, point index) order, without the non-finite ones: d_adjStart (the cell
// table; its last word is the number of binned points), d_adjPerm, d_adjPts.  Scratch grown by the caller before sample_grid.
static int adjoint_bin_grow(SphEngine* e, size_t m, size_t cells) {
    int rc;
    if ((rc = e->d_adjKey.grow(e, m)) || (rc = e->d_adjTmp.grow(e, m)) || (rc = e->d_adjPerm.grow(e, m)) || (rc = e->d_adjPts.grow(e, m)) ||
        (rc = e->d_adjCount.grow(e, cells + 8)) || (rc = e->d_adjSums.grow(e, (size_t)blocks_for(cells, kScanTile) + 1)) ||
        (rc = e->d_adjStart.grow(e, cells + 1))) return rc;
    return SPH_OK;
}
static int adjoint_bin(SphEngine* e, const SimK& k, const float4* devPoints, size_t m) {
    const uint32_t cells = (uint32_t)k.numCells, mm = (uint32_t)m;
    HIP_TRY(hipMemsetAsync(e->d_adjCount.p, 0, (size_t)cells * sizeof(uint32_t), e->stream));
    Timed t(e, SPH_K_OTHER);
    hipLaunchKernelGGL(k_adjoint_bin, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, k, devPoints, e->d_adjKey.p, e->d_adjCount.p, mm);
    launch_cell_scan(e, e->d_adjCount.p, e->d_adjSums.p, e->d_adjStart.p, (int)cells, mm);
    hipLaunchKernelGGL(k_adjoint_scatter, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, (const uint2*)e->d_adjKey.p, (const uint32_t*)e->d_adjStart.p, e->d_adjTmp.p, mm, cells);
    hipLaunchKernelGGL(k_adjoint_rank, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, (const uint2*)e->d_adjKey.p, (const uint32_t*)e->d_adjStart.p,
                       (const uint32_t*)e->d_adjTmp.p, devPoints, e->d_adjPerm.p, e->d_adjPts.p, mm, cells);
    return SPH_OK;
}

// The adjoint (route false: devArg null) or the routing of g.  Grid of the current state, ids, the rows (sorted slots, or the binned
// points), g (and arg) staged into row order, the walk.  No synchronisation: nothing is read back.
static int adjoint_run(SphEngine* e, bool query, bool route, const SphAggregateConfig* cfg, const float4* devPoints, size_t m, const int32_t* devArg,
                       const float* devG, float* devOut, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = adjoint_check(*cfg, g.cellSize, query, route, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, planes = route ? 1 : (size_t)aggregate_planes(*cfg);
    if (n && !devOut) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!devG || (route && !devArg) || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (planes * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, planes, C);
    const size_t gBytes = rows * planes * C * sizeof(float), outBytes = n * C * sizeof(float);
    if (ranges_overlap(devOut, outBytes, devG, gBytes) || ranges_overlap(devOut, outBytes, devArg, route ? rows * C * sizeof(int32_t) : 0) ||
        ranges_overlap(devOut, outBytes, devPoints, query ? m * sizeof(float4) : 0)) return fail(SPH_ERR_ARG, "the output overlaps g, arg or the points");
    SphAggregateInfo info{};
    info.rows = n; info.channels = cfg->channels; info.planes = (int32_t)planes; info.stencil = stencil; info.flags = cfg->flags; info.radius = cfg->radius;
    *out = info;
    if (!n) return SPH_OK;
    if (!rows) {                                                        // no query point: every row is +0
        HIP_TRY(hipMemsetAsync(devOut, 0, outBytes, e->stream));
        return SPH_OK;
    }
    if (!query && !route && planes == 1) {                             // the relation and the weights are symmetric: the forward of g
        SphAggregateInfo fwd;
        return aggregate_run(e, false, cfg, nullptr, 0, devG, devOut, nullptr, &fwd);
    }
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_aggStage.grow(e, rows * planes * C)) || (route && (rc = e->d_adjArg.grow(e, rows * C))) ||
        (query && (rc = adjoint_bin_grow(e, m, (size_t)g.numCells)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const AggK ag{cfg->op, cfg->weight, cfg->channels, 0, 0};
    slot_ids_fill(e);
    if (query && (rc = adjoint_bin(e, k, devPoints, m))) return rc;
    const uint32_t* perm = query ? (const uint32_t*)e->d_adjPerm.p : reinterpret_cast<const uint32_t*>(e->d_slotIds.p);
    const uint32_t* binned = query ? (const uint32_t*)e->d_adjStart.p + k.numCells : nullptr;
    const AdjRows R{query ? (const float4*)e->d_adjPts.p : (const float4*)e->d_sPV, query ? (const uint32_t*)e->d_adjStart.p : (const uint32_t*)e->d_cellStart, (uint32_t)rows};
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_adjoint_stage, dim3(blocks_for(rows * planes * C)), dim3(kBlock), 0, e->stream, perm, binned, reinterpret_cast<const uint32_t*>(devG),
                           reinterpret_cast<uint32_t*>(e->d_aggStage.p), (uint32_t)rows, (int)(planes * C));
        if (route)
            hipLaunchKernelGGL(k_adjoint_stage, dim3(blocks_for(rows * C)), dim3(kBlock), 0, e->stream, perm, binned, reinterpret_cast<const uint32_t*>(devArg),
                               e->d_adjArg.p, (uint32_t)rows, (int)C);
    }
    {
        Timed t(e, SPH_K_OTHER);
        const bool moments = planes == 4, delta = !query && (cfg->flags & SPH_AGGREGATE_DELTA) != 0;
        // (DELTA with MOMENTS keeps the particle's own four planes beside the accumulators: 16 channels per pass need 130 VGPRs, 8 need 90)
        const int chunk = (delta && moments) ? std::min(aggregate_chunk(cfg->channels), 8) : aggregate_chunk(cfg->channels);
        const dim3 grid(blocks_for(n)), block(kBlock);
        const float4 *pv = (const float4*)e->d_sPV, *own = (const float4*)e->d_sOwn;
        const int32_t* ids = (const int32_t*)e->d_slotIds.p;
        if (route) {
            using Kernel = void (*)(SimK, NbK, AggK, const float4*, const int32_t*, const float4*, AdjRows, const int32_t*, const float*, float*);
            auto pick = [&](auto ch) -> Kernel {
                constexpr int CH = decltype(ch)::value;
                return query ? (Kernel)k_aggregate_route<true, CH> : (Kernel)k_aggregate_route<false, CH>;
            };
            const Kernel kernel = chunk == 4 ? pick(std::integral_constant<int, 4>{}) : chunk == 8 ? pick(std::integral_constant<int, 8>{}) : pick(std::integral_constant<int, 16>{});
            hipLaunchKernelGGL(kernel, grid, block, 0, e->stream, k, nb, ag, pv, ids, own, R, reinterpret_cast<const int32_t*>(e->d_adjArg.p), (const float*)e->d_aggStage.p, devOut);
        } else {
            using Kernel = void (*)(SimK, NbK, AggK, const float4*, const int32_t*, const float4*, AdjRows, const float*, float*);
            auto pick = [&](auto ch) -> Kernel {
                constexpr int CH = decltype(ch)::value;
                if (query) return moments ? (Kernel)k_aggregate_adjoint<true, true, false, CH> : (Kernel)k_aggregate_adjoint<true, false, false, CH>;
                return delta ? (Kernel)k_aggregate_adjoint<false, true, true, (CH > 8 ? 8 : CH)> : (Kernel)k_aggregate_adjoint<false, true, false, CH>;
            };
            const Kernel kernel = chunk == 4 ? pick(std::integral_constant<int, 4>{}) : chunk == 8 ? pick(std::integral_constant<int, 8>{}) : pick(std::integral_constant<int, 16>{});
            hipLaunchKernelGGL(kernel, grid, block, 0, e->stream, k, nb, ag, pv, ids, own, R, (const float*)e->d_aggStage.p, devOut);
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_adjoint_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devG, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return adjoint_run(e, false, false, cfg, nullptr, 0, nullptr, devG, devOut, info);
}

int sph_aggregate_adjoint_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devG, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return adjoint_run(e, true, false, cfg, reinterpret_cast<const float4*>(devPoints4), m, nullptr, devG, devOut, info);
}

int sph_aggregate_route_particles(SphEngine* e, const SphAggregateConfig* cfg, const int32_t* devArg, const float* devG, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return adjoint_run(e, false, true, cfg, nullptr, 0, devArg, devG, devOut, info);
}

int sph_aggregate_route_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const int32_t* devArg, const float* devG, float* devOut,
                              SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return adjoint_run(e, true, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devArg, devG, devOut, info);
}

// Host memory in and out through engine scratch, as sph_aggregate_staged: the upload, the device call, the download, one synchronisation.
int sph_aggregate_adjoint_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* g, float* out, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo grid;
    int rc, stencil = 0;
    if ((rc = query_grid(e, grid)) || (rc = adjoint_check(*cfg, grid.cellSize, query, false, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, gWords = rows * (size_t)aggregate_planes(*cfg) * C;
    if (n && (!out || (rows && !g))) return fail(SPH_ERR_ARG, "null argument");
    if (n && ((rc = e->d_adjIn.grow(e, gWords + 1)) || (rc = e->d_aggOut.grow(e, n * C)) || (query && (rc = e->d_sampleIn.grow(e, m + 1))))) return rc;
    if (n && gWords) HIP_TRY(hipMemcpyAsync(e->d_adjIn.p, g, gWords * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && query && m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = adjoint_run(e, query, false, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, nullptr, e->d_adjIn.p, e->d_aggOut.p, info))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(out, e->d_aggOut.p, n * C * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// MAX / MIN with the winners: aggregate_run's order of work; the values are always staged into slot order.
static int arg_run(SphEngine* e, bool query, const SphAggregateConfig* cfg, const float4* devPoints, size_t m, const float* devValues, float* devOut,
                   uint32_t* devCount, int32_t* devArg, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = adjoint_check(*cfg, g.cellSize, query, true, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels;
    if (rows && n && (!devValues || !devOut || !devArg || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu floats exceed size_t", rows, C);
    const size_t outBytes = rows * C * sizeof(float), valBytes = n * C * sizeof(float), cntBytes = devCount ? rows * sizeof(uint32_t) : 0;
    if (ranges_overlap(devOut, outBytes, devValues, valBytes) || ranges_overlap(devCount, cntBytes, devValues, valBytes) || ranges_overlap(devArg, outBytes, devValues, valBytes) ||
        ranges_overlap(devArg, outBytes, devOut, outBytes) || ranges_overlap(devArg, outBytes, devCount, cntBytes) || ranges_overlap(devOut, outBytes, devCount, cntBytes))
        return fail(SPH_ERR_ARG, "the outputs overlap the values or each other");
    SphAggregateInfo info{};
    info.rows = rows; info.channels = cfg->channels; info.planes = 1; info.stencil = stencil; info.flags = cfg->flags; info.radius = cfg->radius;
    *out = info;
    if (!rows || !n) return SPH_OK;
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_aggStage.grow(e, n * C))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const AggK ag{cfg->op, cfg->weight, cfg->channels, 0, 0};
    slot_ids_fill(e);
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * C)), dim3(kBlock), 0, e->stream, (const int32_t*)e->d_slotIds.p, devValues, e->d_aggStage.p, (uint32_t)n, cfg->channels);
    }
    {
        Timed t(e, SPH_K_OTHER);
        using Kernel = void (*)(SimK, NbK, AggK, const float4*, const uint32_t*, const int32_t*, const float4*, const float4*, size_t, const float*, float*, uint32_t*, int32_t*);
        auto pick = [&](auto ch) -> Kernel {
            constexpr int CH = decltype(ch)::value;
            return query ? (Kernel)k_aggregate_arg<false, CH> : (Kernel)k_aggregate_arg<true, CH>;
        };
        const int chunk = aggregate_chunk(cfg->channels);
        const Kernel kernel = chunk == 4 ? pick(std::integral_constant<int, 4>{}) : chunk == 8 ? pick(std::integral_constant<int, 8>{}) : pick(std::integral_constant<int, 16>{});
        hipLaunchKernelGGL(kernel, dim3(blocks_for(rows)), dim3(kBlock), 0, e->stream, k, nb, ag, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                           (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn, devPoints, rows, (const float*)e->d_aggStage.p, devOut, devCount, devArg);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_arg_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, int32_t* devArg,
                                SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return arg_run(e, false, cfg, nullptr, 0, devValues, devOut, devCount, devArg, info);
}

int sph_aggregate_arg_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut, uint32_t* devCount,
                            int32_t* devArg, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return arg_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devValues, devOut, devCount, devArg, info);
}

// What the three host twins open with: the params, the grid they give, the config.
static int adjoint_host_open(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, bool query, size_t m, bool extremum,
                             SimK& k, int* stencil) {
    if (!params || !cfg || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    sph::make_simk(*params, g, params->param_timeStep, k);
    return adjoint_check(*cfg, g.cellSize, query, extremum, stencil);
}

int sph_aggregate_adjoint_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                               const float* g, float* out) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = adjoint_host_open(particles, n, params, cfg, query, m, false, k, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (!n) return SPH_OK;
    if (!out || (rows && !g)) return fail(SPH_ERR_ARG, "null argument");
    if (ranges_overlap(out, n * C * sizeof(float), g, rows * planes * C * sizeof(float)) || ranges_overlap(out, n * C * sizeof(float), points4, query ? m * 4 * sizeof(float) : 0))
        return fail(SPH_ERR_ARG, "the output overlaps g or the points");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const bool delta = !query && (cfg->flags & SPH_AGGREGATE_DELTA) != 0, moments = planes == 4;
    const sph::AdjHostRows table = query ? sph::AdjHostRows(k, points4, m) : sph::AdjHostRows(sph::HostGrid(k, particles, n));
    std::vector<float> acc(C);
    for (size_t r = 0; r < n; ++r) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        const float* mine = delta ? g + r * planes * C : nullptr;
        sph::adjoint_walk_host(k, stencil, table, particles, points4, r, R2, self, fluidOnly, [&](size_t row, float dx, float dy, float dz, float r2) {
            const float* grow = g + row * planes * C;
            const float w = sph::aggregate_weight(cfg->weight, R2, r2);
            for (size_t c = 0; c < C; ++c) {
                acc[c] = sph::aggregate_add(acc[c], w, sph::aggregate_adjoint_plane0(delta, grow[c], delta ? mine[c] : 0.0f));
                if (!moments) continue;
                acc[c] = sph::aggregate_add_moment(acc[c], w, dx, sph::aggregate_adjoint_moment(delta, grow[C + c], delta ? mine[C + c] : 0.0f));
                acc[c] = sph::aggregate_add_moment(acc[c], w, dy, sph::aggregate_adjoint_moment(delta, grow[2 * C + c], delta ? mine[2 * C + c] : 0.0f));
                acc[c] = sph::aggregate_add_moment(acc[c], w, dz, sph::aggregate_adjoint_moment(delta, grow[3 * C + c], delta ? mine[3 * C + c] : 0.0f));
            }
        });
        memcpy(out + r * C, acc.data(), C * sizeof(float));
    }
    return SPH_OK;
}

int sph_aggregate_route_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                             const int32_t* arg, const float* g, float* out) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = adjoint_host_open(particles, n, params, cfg, query, m, true, k, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels;
    if (!n) return SPH_OK;
    if (!out || (rows && (!g || !arg))) return fail(SPH_ERR_ARG, "null argument");
    if (ranges_overlap(out, n * C * sizeof(float), g, rows * C * sizeof(float)) || ranges_overlap(out, n * C * sizeof(float), arg, rows * C * sizeof(int32_t)) ||
        ranges_overlap(out, n * C * sizeof(float), points4, query ? m * 4 * sizeof(float) : 0)) return fail(SPH_ERR_ARG, "the output overlaps g, arg or the points");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const sph::AdjHostRows table = query ? sph::AdjHostRows(k, points4, m) : sph::AdjHostRows(sph::HostGrid(k, particles, n));
    std::vector<float> acc(C);
    for (size_t r = 0; r < n; ++r) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        sph::adjoint_walk_host(k, stencil, table, particles, points4, r, R2, self, fluidOnly, [&](size_t row, float, float, float, float) {
            for (size_t c = 0; c < C; ++c)
                if (arg[row * C + c] == (int32_t)r) acc[c] = acc[c] + g[row * C + c];
        });
        memcpy(out + r * C, acc.data(), C * sizeof(float));
    }
    return SPH_OK;
}

int sph_aggregate_arg_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                           const float* values, float* out, uint32_t* count, int32_t* arg) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = adjoint_host_open(particles, n, params, cfg, query, m, true, k, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels;
    if (!rows || !n) return SPH_OK;
    if (!values || !out || !arg) return fail(SPH_ERR_ARG, "null argument");
    const size_t outBytes = rows * C * sizeof(float), valBytes = n * C * sizeof(float), cntBytes = count ? rows * sizeof(uint32_t) : 0;
    if (ranges_overlap(out, outBytes, values, valBytes) || ranges_overlap(count, cntBytes, values, valBytes) || ranges_overlap(arg, outBytes, values, valBytes) ||
        ranges_overlap(arg, outBytes, out, outBytes) || ranges_overlap(arg, outBytes, count, cntBytes) || ranges_overlap(out, outBytes, count, cntBytes))
        return fail(SPH_ERR_ARG, "the outputs overlap the values or each other");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const bool delta = !query && (cfg->flags & SPH_AGGREGATE_DELTA) != 0, isMax = cfg->op == SPH_AGGREGATE_MAX;
    const sph::HostGrid grid(k, particles, n);
    std::vector<uint32_t> best(C), who(C);
    for (size_t r = 0; r < rows; ++r) {
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
        std::fill(best.begin(), best.end(), isMax ? sph::kAggLowest : sph::kAggHighest);
        std::fill(who.begin(), who.end(), sph::kAggNoArg);
        uint32_t cnt = 0u;
        const float* mine = values + (query ? 0 : r) * C;
        if (walk) {
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    const uint32_t id = grid.order[j];
                    const SphParticle& cand = particles[id];
                    float dx, dy, dz, r2;
                    if (!sph::aggregate_accept(!query && j == grid.slotOf[r], self, x[0], x[1], x[2], cand.pos[0], cand.pos[1], cand.pos[2], R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && cand.isGhost != 0) continue;
                    const float* v = values + (size_t)id * C;
                    cnt += 1u;
                    for (size_t c = 0; c < C; ++c) sph::aggregate_arg_step(isMax, best[c], who[c], sph::aggregate_value(delta, v[c], mine[c]), id);
                }
            });
        }
        for (size_t c = 0; c < C; ++c) {
            out[r * C + c] = sph::agg_unordered(best[c]);
            arg[r * C + c] = who[c] == sph::kAggNoArg ? -1 : (int32_t)who[c];
        }
        if (count) count[r] = cnt;
    }
    return SPH_OK;
}

// ---- filter-grid basis sums and their adjoint (sph_conv.h) ----------------------
static_assert(sizeof(SphBasisConfig) == 32, "SphBasisConfig is 32 bytes");
static_assert(SPH_BASIS_GRID == sph::kBasisGrid, "sph_conv.h mirrors SPH_BASIS_*");

void sph_aggregate_basis_default(SphBasisConfig* cfg) {
    if (!cfg) return;
    *cfg = SphBasisConfig{};
    cfg->weight = SPH_AGGREGATE_WEIGHT_POLY6;
    cfg->channels = 1;
    cfg->kind = SPH_BASIS_GRID;
    cfg->size = 4;
}

// The config as an argument: the stencil half-width through *stencil.
static int basis_check(const SphBasisConfig& c, float cellSize, bool query, int* stencil) {
    if (c.weight < SPH_AGGREGATE_WEIGHT_ONE || c.weight > SPH_AGGREGATE_WEIGHT_POLY6) return fail(SPH_ERR_ARG, "unknown basis weight %d", c.weight);
    if (c.flags & (SPH_AGGREGATE_DELTA | SPH_AGGREGATE_MOMENTS)) return fail(SPH_ERR_ARG, "SPH_AGGREGATE_DELTA / _MOMENTS do not apply to basis sums (flags %d)", c.flags);
    if (c.flags & ~(SPH_AGGREGATE_SELF | SPH_AGGREGATE_FLUID_ONLY)) return fail(SPH_ERR_ARG, "unknown basis flags %d", c.flags);
    if (c.pad[0] || c.pad[1]) return fail(SPH_ERR_ARG, "the padding of SphBasisConfig must be zero");
    if (c.channels < 1 || c.channels > SPH_AGGREGATE_MAX_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (1 .. %d)", c.channels, (int)SPH_AGGREGATE_MAX_CHANNELS);
    if (c.kind != SPH_BASIS_GRID) return fail(SPH_ERR_ARG, "unknown basis kind %d", c.kind);
    if (c.size < sph::kBasisMinSize || c.size > sph::kBasisMaxSize) return fail(SPH_ERR_ARG, "filter grid size %d (%d .. %d)", c.size, sph::kBasisMinSize, sph::kBasisMaxSize);
    if (query && (c.flags & SPH_AGGREGATE_SELF)) return fail(SPH_ERR_ARG, "SPH_AGGREGATE_SELF applies to particle targets only");
    return radius_stencil(c.radius, cellSize, stencil);
}

static size_t basis_planes(const SphBasisConfig& c) { return (size_t)(c.size * c.size * c.size); }
static sph::BasisK make_basisk(const SphBasisConfig& c) {
    return sph::BasisK{c.radius, 0.5f * (float)(c.size - 1), c.weight, c.channels, c.size, sph::basis_group_shift(c.channels)};
}
static void basis_info(const SphBasisConfig& c, size_t rows, int stencil, SphAggregateInfo* out) {
    SphAggregateInfo info{};
    info.rows = rows; info.channels = c.channels; info.planes = (int32_t)basis_planes(c); info.stencil = stencil; info.flags = c.flags; info.radius = c.radius;
    *out = info;
}

// Grid of the current state, ids, the stage, the walk.  No synchronisation: nothing is read back.
static int basis_run(SphEngine* e, bool query, const SphBasisConfig* cfg, const float4* devPoints, size_t m, const float* devValues, float* devOut,
                     uint32_t* devCount, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = basis_check(*cfg, g.cellSize, query, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (rows && n && (!devValues || !devOut || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t outBytes = rows * B * C * sizeof(float), valBytes = n * C * sizeof(float);
    if (ranges_overlap(devOut, outBytes, devValues, valBytes) || ranges_overlap(devCount, devCount ? rows * sizeof(uint32_t) : 0, devValues, valBytes))
        return fail(SPH_ERR_ARG, "the output overlaps the values");
    basis_info(*cfg, rows, stencil, out);
    if (!rows || !n) return SPH_OK;
    if ((rc = e->d_slotIds.grow(e, n)) || (rc = e->d_aggStage.grow(e, n * C))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const BasisK bk = make_basisk(*cfg);
    slot_ids_fill(e);
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * C)), dim3(kBlock), 0, e->stream, (const int32_t*)e->d_slotIds.p, devValues, e->d_aggStage.p, (uint32_t)n, cfg->channels);
    }
    {
        Timed t(e, SPH_K_OTHER);
        const int block = basis_block(cfg->size);
        const size_t lds = B * (size_t)block * sizeof(float);
        auto kernel = query ? k_aggregate_basis<false> : k_aggregate_basis<true>;
        hipLaunchKernelGGL(kernel, dim3(blocks_for(rows << bk.gshift, block)), dim3(block), lds, e->stream, k, nb, bk, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart,
                           (const int32_t*)e->d_slotIds.p, (const float4*)e->d_sOwn, devPoints, rows, (const float*)e->d_aggStage.p, devOut, devCount);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_basis_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devValues, float* devOut, uint32_t* devCount, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return basis_run(e, false, cfg, nullptr, 0, devValues, devOut, devCount, info);
}

int sph_aggregate_basis_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devValues, float* devOut,
                              uint32_t* devCount, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return basis_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devValues, devOut, devCount, info);
}

// Host memory in and out through engine scratch, as sph_aggregate_staged: the upload, the device call, the download, one synchronisation.
int sph_aggregate_basis_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* values, float* out, uint32_t* count,
                               SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = basis_check(*cfg, g.cellSize, query, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t cells = rows * B * C;
    const bool work = rows && n;
    if (work && (!values || !out)) return fail(SPH_ERR_ARG, "null argument");
    if (work && ((rc = e->d_aggIn.grow(e, n * C)) || (rc = e->d_aggOut.grow(e, cells)) || (rc = e->d_aggCnt.grow(e, rows)) ||
                 (query && (rc = e->d_sampleIn.grow(e, m))))) return rc;
    if (work) HIP_TRY(hipMemcpyAsync(e->d_aggIn.p, values, n * C * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (work && query) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = basis_run(e, query, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, e->d_aggIn.p, e->d_aggOut.p,
                        count ? e->d_aggCnt.p : nullptr, info))) return rc;
    if (work) HIP_TRY(hipMemcpyAsync(out, e->d_aggOut.p, cells * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (work && count) HIP_TRY(hipMemcpyAsync(count, e->d_aggCnt.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// What the two host twins open with: the params, the grid they give, the config.
static int basis_host_open(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, bool query, size_t m, SimK& k, int* stencil) {
    if (!params || !cfg || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    sph::make_simk(*params, g, params->param_timeStep, k);
    return basis_check(*cfg, g.cellSize, query, stencil);
}

int sph_aggregate_basis_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                             const float* values, float* out, uint32_t* count) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = basis_host_open(particles, n, params, cfg, query, m, k, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (!rows || !n) return SPH_OK;
    if (!values || !out) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    if (ranges_overlap(out, rows * B * C * sizeof(float), values, n * C * sizeof(float)) ||
        ranges_overlap(count, count ? rows * sizeof(uint32_t) : 0, values, n * C * sizeof(float))) return fail(SPH_ERR_ARG, "the output overlaps the values");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const sph::BasisK bk = make_basisk(*cfg);
    const sph::HostGrid grid(k, particles, n);
    std::vector<float> acc(B * C);
    for (size_t r = 0; r < rows; ++r) {
        const float* x = query ? points4 + 4 * r : particles[r].pos;
        const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
        std::fill(acc.begin(), acc.end(), 0.0f);
        uint32_t cnt = 0u;
        if (walk) {
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    const SphParticle& cand = particles[grid.order[j]];
                    float dx, dy, dz, r2;
                    if (!sph::aggregate_accept(!query && j == grid.slotOf[r], self, x[0], x[1], x[2], cand.pos[0], cand.pos[1], cand.pos[2], R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && cand.isGhost != 0) continue;
                    const float* v = values + (size_t)grid.order[j] * C;
                    const float w = sph::aggregate_weight(cfg->weight, R2, r2);
                    int b[8];
                    float coef[8];
                    sph::basis_corners(bk.R, bk.half, bk.K, w, dx, dy, dz, b, coef);
                    cnt += 1u;
                    for (int t = 0; t < 8; ++t) {
                        float* plane = acc.data() + (size_t)b[t] * C;
                        for (size_t c = 0; c < C; ++c) plane[c] = sph::basis_add(plane[c], coef[t], v[c]);
                    }
                }
            });
        }
        memcpy(out + r * B * C, acc.data(), B * C * sizeof(float));
        if (count) count[r] = cnt;
    }
    return SPH_OK;
}

// The adjoint.  Grid of the current state, ids, the rows (sorted slots, or the binned points), the walk; h is read in place through
// ids[] / perm[].  No synchronisation: nothing is read back.
static int basis_adjoint_run(SphEngine* e, bool query, const SphBasisConfig* cfg, const float4* devPoints, size_t m, const float* devH, float* devOut,
                             SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = basis_check(*cfg, g.cellSize, query, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (n && !devOut) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!devH || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t hBytes = rows * B * C * sizeof(float), outBytes = n * C * sizeof(float);
    if (ranges_overlap(devOut, outBytes, devH, hBytes) || ranges_overlap(devOut, outBytes, devPoints, query ? m * sizeof(float4) : 0))
        return fail(SPH_ERR_ARG, "the output overlaps h or the points");
    basis_info(*cfg, n, stencil, out);
    if (!n) return SPH_OK;
    if (!rows) {                                                        // no query point: every row is +0
        HIP_TRY(hipMemsetAsync(devOut, 0, outBytes, e->stream));
        return SPH_OK;
    }
    if ((rc = e->d_slotIds.grow(e, n)) || (query && (rc = adjoint_bin_grow(e, m, (size_t)g.numCells)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const BasisK bk = make_basisk(*cfg);
    slot_ids_fill(e);
    if (query && (rc = adjoint_bin(e, k, devPoints, m))) return rc;
    const uint32_t* rowOf = query ? (const uint32_t*)e->d_adjPerm.p : reinterpret_cast<const uint32_t*>(e->d_slotIds.p);
    const AdjRows R{query ? (const float4*)e->d_adjPts.p : (const float4*)e->d_sPV, query ? (const uint32_t*)e->d_adjStart.p : (const uint32_t*)e->d_cellStart, (uint32_t)rows};
    {
        Timed t(e, SPH_K_OTHER);
        auto kernel = query ? k_aggregate_basis_adjoint<true> : k_aggregate_basis_adjoint<false>;
        hipLaunchKernelGGL(kernel, dim3(blocks_for(n << bk.gshift)), dim3(kBlock), 0, e->stream, k, nb, bk, (const float4*)e->d_sPV, (const int32_t*)e->d_slotIds.p,
                           (const float4*)e->d_sOwn, R, rowOf, devH, devOut);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_basis_adjoint_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devH, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return basis_adjoint_run(e, false, cfg, nullptr, 0, devH, devOut, info);
}

int sph_aggregate_basis_adjoint_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devH, float* devOut,
                                      SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return basis_adjoint_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devH, devOut, info);
}

int sph_aggregate_basis_adjoint_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* h, float* out, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo grid;
    int rc, stencil = 0;
    if ((rc = query_grid(e, grid)) || (rc = basis_check(*cfg, grid.cellSize, query, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t hWords = rows * B * C;
    if (n && (!out || (rows && !h))) return fail(SPH_ERR_ARG, "null argument");
    if (n && ((rc = e->d_adjIn.grow(e, hWords + 1)) || (rc = e->d_aggOut.grow(e, n * C)) || (query && (rc = e->d_sampleIn.grow(e, m + 1))))) return rc;
    if (n && hWords) HIP_TRY(hipMemcpyAsync(e->d_adjIn.p, h, hWords * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && query && m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = basis_adjoint_run(e, query, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, e->d_adjIn.p, e->d_aggOut.p, info))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(out, e->d_aggOut.p, n * C * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_aggregate_basis_adjoint_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                                     const float* h, float* out) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = basis_host_open(particles, n, params, cfg, query, m, k, &stencil))) return rc;
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (!n) return SPH_OK;
    if (!out || (rows && !h)) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    if (ranges_overlap(out, n * C * sizeof(float), h, rows * B * C * sizeof(float)) || ranges_overlap(out, n * C * sizeof(float), points4, query ? m * 4 * sizeof(float) : 0))
        return fail(SPH_ERR_ARG, "the output overlaps h or the points");
    const float R2 = cfg->radius * cfg->radius;
    const bool self = (cfg->flags & SPH_AGGREGATE_SELF) != 0, fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const sph::BasisK bk = make_basisk(*cfg);
    const sph::AdjHostRows table = query ? sph::AdjHostRows(k, points4, m) : sph::AdjHostRows(sph::HostGrid(k, particles, n));
    std::vector<float> acc(C);
    for (size_t r = 0; r < n; ++r) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        sph::adjoint_walk_host(k, stencil, table, particles, points4, r, R2, self, fluidOnly, [&](size_t row, float dx, float dy, float dz, float r2) {
            const float* hrow = h + row * B * C;
            const float w = sph::aggregate_weight(cfg->weight, R2, r2);
            int b[8];
            float coef[8];
            sph::basis_corners(bk.R, bk.half, bk.K, w, dx, dy, dz, b, coef);
            for (size_t c = 0; c < C; ++c)
                for (int t = 0; t < 8; ++t) acc[c] = sph::basis_add(acc[c], coef[t], hrow[(size_t)b[t] * C + c]);
        });
        memcpy(out + r * C, acc.data(), C * sizeof(float));
    }
    return SPH_OK;
}

// ---- position gradients of the neighbourhood sums (sph_posgrad.h) ----------------
// Do the outputs (either may be null) share an address with an input or with each other?
static bool posgrad_overlap(const float* outPoints, size_t ptBytes, const float* outParticles, size_t paBytes, const void* values, size_t valBytes, const void* g,
                            size_t gBytes, const void* points, size_t pointBytes) {
    const float* outs[2] = {outPoints, outParticles};
    const size_t bytes[2] = {outPoints ? ptBytes : 0, outParticles ? paBytes : 0};
    for (int o = 0; o < 2; ++o)
        if (ranges_overlap(outs[o], bytes[o], values, valBytes) || ranges_overlap(outs[o], bytes[o], g, gBytes) || ranges_overlap(outs[o], bytes[o], points, pointBytes))
            return true;
    return ranges_overlap(outs[0], bytes[0], outs[1], bytes[1]);
}
// Has the config no dependence on the positions?  (ONE without MOMENTS: out is a plain sum of values; its cutoff is not differentiated.)
static bool posgrad_constant(const SphAggregateConfig& c) { return c.weight == SPH_AGGREGATE_WEIGHT_ONE && !(c.flags & SPH_AGGREGATE_MOMENTS); }

// Grid of the current state, ids, the stages (values and g into slot order; for the particles' side of query targets the points binned
// and g into binned order), the walks.  Query targets: a null output's walk is not launched.  No synchronisation.
static int posgrad_run(SphEngine* e, bool query, const SphAggregateConfig* cfg, const float4* devPoints, size_t m, const float* devValues, const float* devG,
                       float* devOutPoints, float* devOutParticles, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = adjoint_check(*cfg, g.cellSize, query, false, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    if (query && !devOutPoints && !devOutParticles) return fail(SPH_ERR_ARG, "both outputs are null");
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (!query && n && !devOutParticles) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!devValues || !devG || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (planes * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, planes, C);
    const size_t gBytes = rows * planes * C * sizeof(float), valBytes = n * C * sizeof(float), ptBytes = query ? m * 3 * sizeof(float) : 0, paBytes = n * 3 * sizeof(float);
    if (posgrad_overlap(query ? devOutPoints : nullptr, ptBytes, devOutParticles, paBytes, devValues, valBytes, devG, gBytes, devPoints, query ? m * sizeof(float4) : 0))
        return fail(SPH_ERR_ARG, "an output overlaps the values, g, the points or the other output");
    SphAggregateInfo info{};
    info.rows = rows; info.channels = cfg->channels; info.planes = (int32_t)planes; info.stencil = stencil; info.flags = cfg->flags; info.radius = cfg->radius;
    *out = info;
    if (!n) return SPH_OK;
    if (!rows || posgrad_constant(*cfg)) {                               // no query point, or nothing depends on the positions: every row is +0
        if (devOutParticles) HIP_TRY(hipMemsetAsync(devOutParticles, 0, paBytes, e->stream));
        if (query && devOutPoints && rows) HIP_TRY(hipMemsetAsync(devOutPoints, 0, ptBytes, e->stream));
        return SPH_OK;
    }
    const bool targets = !query || devOutPoints, candidates = query && devOutParticles;
    if ((rc = e->d_slotIds.grow(e, n)) || (targets && (rc = e->d_aggStage.grow(e, n * C))) || ((!query || candidates) && (rc = e->d_posStage.grow(e, rows * planes * C))) ||
        (candidates && (rc = adjoint_bin_grow(e, m, (size_t)g.numCells)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const PosK pk{cfg->weight, cfg->channels, (!query && (cfg->flags & SPH_AGGREGATE_DELTA)) ? 1 : 0, posgrad_group_shift(cfg->channels)};
    const bool moments = planes == 4, two = cfg->channels > kPosMaxGroup;
    slot_ids_fill(e);
    if (candidates && (rc = adjoint_bin(e, k, devPoints, m))) return rc;
    const int32_t* ids = (const int32_t*)e->d_slotIds.p;
    {
        Timed t(e, SPH_K_OTHER);
        if (targets) hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * C)), dim3(kBlock), 0, e->stream, ids, devValues, e->d_aggStage.p, (uint32_t)n, cfg->channels);
        if (!query)
            hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * planes * C)), dim3(kBlock), 0, e->stream, ids, devG, e->d_posStage.p, (uint32_t)n, (int)(planes * C));
        if (candidates)
            hipLaunchKernelGGL(k_adjoint_stage, dim3(blocks_for(m * planes * C)), dim3(kBlock), 0, e->stream, (const uint32_t*)e->d_adjPerm.p,
                               (const uint32_t*)e->d_adjStart.p + k.numCells, reinterpret_cast<const uint32_t*>(devG), reinterpret_cast<uint32_t*>(e->d_posStage.p),
                               (uint32_t)m, (int)(planes * C));
    }
    using Kernel = void (*)(SimK, NbK, PosK, const float4*, const uint32_t*, const int32_t*, const float4*, const float4*, size_t, AdjRows, const float*, const float*, float*);
    auto pick = [&](auto mode) -> Kernel {
        constexpr int MODE = decltype(mode)::value;
        if (moments) return two ? (Kernel)k_aggregate_posgrad<MODE, true, 2> : (Kernel)k_aggregate_posgrad<MODE, true, 1>;
        return two ? (Kernel)k_aggregate_posgrad<MODE, false, 2> : (Kernel)k_aggregate_posgrad<MODE, false, 1>;
    };
    const float4 *pv = (const float4*)e->d_sPV, *own = (const float4*)e->d_sOwn;
    const uint32_t* cellStart = (const uint32_t*)e->d_cellStart;
    const AdjRows none{nullptr, nullptr, 0u};
    {
        Timed t(e, SPH_K_OTHER);
        if (!query)
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosParticles>{}), dim3(blocks_for(n << pk.gshift)), dim3(kBlock), 0, e->stream, k, nb, pk, pv, cellStart, ids,
                               own, (const float4*)nullptr, n, none, (const float*)e->d_aggStage.p, (const float*)e->d_posStage.p, devOutParticles);
        if (query && targets)
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosPoints>{}), dim3(blocks_for(m << pk.gshift)), dim3(kBlock), 0, e->stream, k, nb, pk, pv, cellStart, ids,
                               own, devPoints, m, none, (const float*)e->d_aggStage.p, devG, devOutPoints);
        if (candidates) {
            const AdjRows R{(const float4*)e->d_adjPts.p, (const uint32_t*)e->d_adjStart.p, (uint32_t)m};
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosCandidates>{}), dim3(blocks_for(n << pk.gshift)), dim3(kBlock), 0, e->stream, k, nb, pk, pv, cellStart,
                               ids, own, (const float4*)nullptr, n, R, devValues, (const float*)e->d_posStage.p, devOutParticles);
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_posgrad_particles(SphEngine* e, const SphAggregateConfig* cfg, const float* devValues, const float* devG, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return posgrad_run(e, false, cfg, nullptr, 0, devValues, devG, nullptr, devOut, info);
}

int sph_aggregate_posgrad_query(SphEngine* e, const SphAggregateConfig* cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                float* devOutPoints, float* devOutParticles, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return posgrad_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devValues, devG, devOutPoints, devOutParticles, info);
}

// Host memory in and out through engine scratch, as sph_aggregate_adjoint_staged: the uploads, the device call, the downloads, one
// synchronisation.  d_aggOut holds the points' rows, then the particles'.
int sph_aggregate_posgrad_staged(SphEngine* e, const SphAggregateConfig* cfg, const float* points4, size_t m, const float* values, const float* g, float* outPoints,
                                 float* outParticles, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo grid;
    int rc, stencil = 0;
    if ((rc = query_grid(e, grid)) || (rc = adjoint_check(*cfg, grid.cellSize, query, false, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    if (query ? (!outPoints && !outParticles) : (e->n && !outParticles)) return fail(SPH_ERR_ARG, query ? "both outputs are null" : "null argument");
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (rows > ((size_t)-1) / (planes * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, planes, C);
    const size_t gWords = rows * planes * C, ptWords = query ? m * 3 : 0;
    if (n && rows && (!values || !g)) return fail(SPH_ERR_ARG, "null argument");
    if (n && ((rc = e->d_aggIn.grow(e, n * C)) || (rc = e->d_adjIn.grow(e, gWords + 1)) || (rc = e->d_aggOut.grow(e, ptWords + n * 3)) ||
              (query && (rc = e->d_sampleIn.grow(e, m + 1))))) return rc;
    if (n && rows) HIP_TRY(hipMemcpyAsync(e->d_aggIn.p, values, n * C * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && gWords) HIP_TRY(hipMemcpyAsync(e->d_adjIn.p, g, gWords * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && query && m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    float *dPoints = (n && query && outPoints) ? e->d_aggOut.p : nullptr, *dParticles = (n && outParticles) ? e->d_aggOut.p + ptWords : nullptr;
    if (!n) { dPoints = outPoints; dParticles = outParticles; }         // (nothing is written: only the null checks read them)
    if ((rc = posgrad_run(e, query, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, e->d_aggIn.p, e->d_adjIn.p, dPoints, dParticles, info))) return rc;
    if (n && dPoints && ptWords) HIP_TRY(hipMemcpyAsync(outPoints, dPoints, ptWords * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (n && dParticles) HIP_TRY(hipMemcpyAsync(outParticles, dParticles, n * 3 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_aggregate_posgrad_host(const SphParticle* particles, size_t n, const SphParams* params, const SphAggregateConfig* cfg, const float* points4, size_t m,
                               const float* values, const float* g, float* outPoints, float* outParticles) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = adjoint_host_open(particles, n, params, cfg, query, m, false, k, &stencil))) return rc;
    if (query && !outPoints && !outParticles) return fail(SPH_ERR_ARG, "both outputs are null");
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, planes = (size_t)aggregate_planes(*cfg);
    if (!query && n && !outParticles) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!values || !g)) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (planes * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, planes, C);
    if (posgrad_overlap(query ? outPoints : nullptr, query ? m * 3 * sizeof(float) : 0, outParticles, n * 3 * sizeof(float), values, n * C * sizeof(float), g,
                        rows * planes * C * sizeof(float), points4, query ? m * 4 * sizeof(float) : 0))
        return fail(SPH_ERR_ARG, "an output overlaps the values, g, the points or the other output");
    if (!n) return SPH_OK;
    if (outParticles) memset(outParticles, 0, n * 3 * sizeof(float));
    if (query && outPoints && m) memset(outPoints, 0, m * 3 * sizeof(float));
    if (!rows || posgrad_constant(*cfg)) return SPH_OK;
    const float R2 = cfg->radius * cfg->radius;
    const bool fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0, delta = !query && (cfg->flags & SPH_AGGREGATE_DELTA) != 0, moments = planes == 4;
    const int Ci = cfg->channels, P = (int)planes;
    const sph::HostGrid grid(k, particles, n);
    if (!query || outPoints) {
        for (size_t r = 0; r < rows; ++r) {
            const float* x = query ? points4 + 4 * r : particles[r].pos;
            const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
            if (!walk) continue;
            float acc[3] = {0.0f, 0.0f, 0.0f};
            const float* gr = g + r * planes * C;
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    if (!query && j == grid.slotOf[r]) continue;          // the own slot's two terms are equal
                    const size_t ci = grid.order[j];
                    const SphParticle& cand = particles[ci];
                    float dx, dy, dz, r2;
                    if (!sph::aggregate_accept(false, false, x[0], x[1], x[2], cand.pos[0], cand.pos[1], cand.pos[2], R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && cand.isGhost != 0) continue;
                    const float* vj = values + ci * C;
                    float s[4], e[3];
                    sph::posgrad_dots_host(Ci, P, delta, gr, vj, query ? nullptr : values + r * C, s);
                    sph::posgrad_pair(moments, cfg->weight, R2, r2, dx, dy, dz, s, e);
                    if (query) {
                        for (int a = 0; a < 3; ++a) acc[a] = acc[a] - e[a];
                    } else {
                        float b[3];
                        sph::posgrad_dots_host(Ci, P, delta, g + ci * planes * C, values + r * C, vj, s);
                        sph::posgrad_pair(moments, cfg->weight, R2, r2, -dx, -dy, -dz, s, b);
                        for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (b[a] - e[a]);
                    }
                }
            });
            memcpy((query ? outPoints : outParticles) + r * 3, acc, sizeof(acc));
        }
    }
    if (query && outParticles) {
        const sph::AdjHostRows table(k, points4, m);
        for (size_t r = 0; r < n; ++r) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            sph::adjoint_walk_host(k, stencil, table, particles, points4, r, R2, false, fluidOnly, [&](size_t row, float dx, float dy, float dz, float r2) {
                float s[4], e[3];
                sph::posgrad_dots_host(Ci, P, false, g + row * planes * C, values + r * C, nullptr, s);
                sph::posgrad_pair(moments, cfg->weight, R2, r2, dx, dy, dz, s, e);
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + e[a];
            });
            memcpy(outParticles + r * 3, acc, sizeof(acc));
        }
    }
    return SPH_OK;
}

// ---- position gradients of the basis sums (sph_convgrad.h) ----------------------
// Grid of the current state, ids, the stage (values into slot order; for the particles' side of query targets the points binned), the
// walks; g is read in place.  Query targets: a null output's walk is not launched.  No synchronisation.
static int convgrad_run(SphEngine* e, bool query, const SphBasisConfig* cfg, const float4* devPoints, size_t m, const float* devValues, const float* devG,
                        float* devOutPoints, float* devOutParticles, SphAggregateInfo* out) {
    using namespace sph;
    SimK k;
    SphGridInfo g;
    int rc, stencil = 0;
    if ((rc = query_grid(e, g)) || (rc = basis_check(*cfg, g.cellSize, query, &stencil))) return rc;
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    if (query && !devOutPoints && !devOutParticles) return fail(SPH_ERR_ARG, "both outputs are null");
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (!query && n && !devOutParticles) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!devValues || !devG || (query && !devPoints))) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t gBytes = rows * B * C * sizeof(float), valBytes = n * C * sizeof(float), ptBytes = query ? m * 3 * sizeof(float) : 0, paBytes = n * 3 * sizeof(float);
    if (posgrad_overlap(query ? devOutPoints : nullptr, ptBytes, devOutParticles, paBytes, devValues, valBytes, devG, gBytes, devPoints, query ? m * sizeof(float4) : 0))
        return fail(SPH_ERR_ARG, "an output overlaps the values, g, the points or the other output");
    basis_info(*cfg, rows, stencil, out);
    if (!n) return SPH_OK;
    if (!rows) {                                                        // no query point: every row is +0
        if (devOutParticles) HIP_TRY(hipMemsetAsync(devOutParticles, 0, paBytes, e->stream));
        return SPH_OK;
    }
    const bool targets = !query || devOutPoints, candidates = query && devOutParticles;
    if ((rc = e->d_slotIds.grow(e, n)) || (targets && (rc = e->d_aggStage.grow(e, n * C))) || (candidates && (rc = adjoint_bin_grow(e, m, (size_t)g.numCells)))) return rc;
    if ((rc = sample_grid(e, k))) return rc;
    const NbK nb = make_nbk(e, cfg->radius, stencil, cfg->flags, e->n);
    const BasisK bk = make_basisk(*cfg);
    const bool two = cfg->channels > kPosMaxGroup;
    slot_ids_fill(e);
    if (candidates && (rc = adjoint_bin(e, k, devPoints, m))) return rc;
    const int32_t* ids = (const int32_t*)e->d_slotIds.p;
    if (targets) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_aggregate_stage, dim3(blocks_for(n * C)), dim3(kBlock), 0, e->stream, ids, devValues, e->d_aggStage.p, (uint32_t)n, cfg->channels);
    }
    const float4 *pv = (const float4*)e->d_sPV, *own = (const float4*)e->d_sOwn;
    const uint32_t* cellStart = (const uint32_t*)e->d_cellStart;
    const AdjRows none{nullptr, nullptr, 0u};
    auto pick = [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        return two ? k_aggregate_basis_posgrad<MODE, 2> : k_aggregate_basis_posgrad<MODE, 1>;
    };
    {
        Timed t(e, SPH_K_OTHER);
        if (!query)
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosParticles>{}), dim3(blocks_for(n << bk.gshift)), dim3(kBlock), 0,
                               e->stream, k, nb, bk, pv, cellStart, ids, own, (const float4*)nullptr, n, none, reinterpret_cast<const uint32_t*>(ids),
                               (const float*)e->d_aggStage.p, devG, devOutParticles);
        if (query && targets)
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosPoints>{}), dim3(blocks_for(m << bk.gshift)), dim3(kBlock), 0,
                               e->stream, k, nb, bk, pv, cellStart, ids, own, devPoints, m, none, (const uint32_t*)nullptr, (const float*)e->d_aggStage.p, devG, devOutPoints);
        if (candidates) {
            const AdjRows R{(const float4*)e->d_adjPts.p, (const uint32_t*)e->d_adjStart.p, (uint32_t)m};
            hipLaunchKernelGGL(pick(std::integral_constant<int, kPosCandidates>{}), dim3(blocks_for(n << bk.gshift)), dim3(kBlock),
                               0, e->stream, k, nb, bk, pv, cellStart, ids, own, (const float4*)nullptr, n, R, (const uint32_t*)e->d_adjPerm.p, devValues, devG, devOutParticles);
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_aggregate_basis_posgrad_particles(SphEngine* e, const SphBasisConfig* cfg, const float* devValues, const float* devG, float* devOut, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return convgrad_run(e, false, cfg, nullptr, 0, devValues, devG, nullptr, devOut, info);
}

int sph_aggregate_basis_posgrad_query(SphEngine* e, const SphBasisConfig* cfg, const float* devPoints4, size_t m, const float* devValues, const float* devG,
                                      float* devOutPoints, float* devOutParticles, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    return convgrad_run(e, true, cfg, reinterpret_cast<const float4*>(devPoints4), m, devValues, devG, devOutPoints, devOutParticles, info);
}

// Host memory in and out through engine scratch, as sph_aggregate_posgrad_staged: the uploads, the device call, the downloads, one
// synchronisation.  d_aggOut holds the points' rows, then the particles'.
int sph_aggregate_basis_posgrad_staged(SphEngine* e, const SphBasisConfig* cfg, const float* points4, size_t m, const float* values, const float* g, float* outPoints,
                                       float* outParticles, SphAggregateInfo* info) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!cfg || !info) return fail(SPH_ERR_ARG, "null argument");
    const bool query = points4 != nullptr;
    SphGridInfo grid;
    int rc, stencil = 0;
    if ((rc = query_grid(e, grid)) || (rc = basis_check(*cfg, grid.cellSize, query, &stencil))) return rc;     // (the refusal, before any allocation)
    if (query && m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu query points (at most 2^31 - 1)", m);
    if (query ? (!outPoints && !outParticles) : (e->n && !outParticles)) return fail(SPH_ERR_ARG, query ? "both outputs are null" : "null argument");
    const size_t n = e->n, rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    const size_t gWords = rows * B * C, ptWords = query ? m * 3 : 0;
    if (n && rows && (!values || !g)) return fail(SPH_ERR_ARG, "null argument");
    if (n && ((rc = e->d_aggIn.grow(e, n * C)) || (rc = e->d_adjIn.grow(e, gWords + 1)) || (rc = e->d_aggOut.grow(e, ptWords + n * 3)) ||
              (query && (rc = e->d_sampleIn.grow(e, m + 1))))) return rc;
    if (n && rows) HIP_TRY(hipMemcpyAsync(e->d_aggIn.p, values, n * C * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && gWords) HIP_TRY(hipMemcpyAsync(e->d_adjIn.p, g, gWords * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (n && query && m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    float *dPoints = (n && query && outPoints) ? e->d_aggOut.p : nullptr, *dParticles = (n && outParticles) ? e->d_aggOut.p + ptWords : nullptr;
    if (!n) { dPoints = outPoints; dParticles = outParticles; }         // (nothing is written: only the null checks read them)
    if ((rc = convgrad_run(e, query, cfg, query ? (const float4*)e->d_sampleIn.p : nullptr, query ? m : 0, e->d_aggIn.p, e->d_adjIn.p, dPoints, dParticles, info))) return rc;
    if (n && dPoints && ptWords) HIP_TRY(hipMemcpyAsync(outPoints, dPoints, ptWords * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (n && dParticles) HIP_TRY(hipMemcpyAsync(outParticles, dParticles, n * 3 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_aggregate_basis_posgrad_host(const SphParticle* particles, size_t n, const SphParams* params, const SphBasisConfig* cfg, const float* points4, size_t m,
                                     const float* values, const float* g, float* outPoints, float* outParticles) {
    const bool query = points4 != nullptr;
    SimK k;
    int rc, stencil = 0;
    if ((rc = basis_host_open(particles, n, params, cfg, query, m, k, &stencil))) return rc;
    if (query && !outPoints && !outParticles) return fail(SPH_ERR_ARG, "both outputs are null");
    const size_t rows = query ? m : n, C = (size_t)cfg->channels, B = basis_planes(*cfg);
    if (!query && n && !outParticles) return fail(SPH_ERR_ARG, "null argument");
    if (n && rows && (!values || !g)) return fail(SPH_ERR_ARG, "null argument");
    if (rows > ((size_t)-1) / (B * C * sizeof(float))) return fail(SPH_ERR_ARG, "%zu rows of %zu x %zu floats exceed size_t", rows, B, C);
    if (posgrad_overlap(query ? outPoints : nullptr, query ? m * 3 * sizeof(float) : 0, outParticles, n * 3 * sizeof(float), values, n * C * sizeof(float), g,
                        rows * B * C * sizeof(float), points4, query ? m * 4 * sizeof(float) : 0))
        return fail(SPH_ERR_ARG, "an output overlaps the values, g, the points or the other output");
    if (!n) return SPH_OK;
    if (outParticles) memset(outParticles, 0, n * 3 * sizeof(float));
    if (query && outPoints && m) memset(outPoints, 0, m * 3 * sizeof(float));
    if (!rows) return SPH_OK;
    const float R2 = cfg->radius * cfg->radius;
    const bool fluidOnly = (cfg->flags & SPH_AGGREGATE_FLUID_ONLY) != 0;
    const sph::BasisK bk = make_basisk(*cfg);
    const sph::HostGrid grid(k, particles, n);
    if (!query || outPoints) {
        for (size_t r = 0; r < rows; ++r) {
            const float* x = query ? points4 + 4 * r : particles[r].pos;
            const bool walk = query ? (sph::float_finite(x[0]) && sph::float_finite(x[1]) && sph::float_finite(x[2])) : !(fluidOnly && particles[r].isGhost != 0);
            if (!walk) continue;
            float acc[3] = {0.0f, 0.0f, 0.0f};
            const float* gr = g + r * B * C;
            grid.rows(stencil, x, [&](uint32_t qs, uint32_t qe) {
                for (uint32_t j = qs; j < qe; ++j) {
                    if (!query && j == grid.slotOf[r]) continue;          // the own slot: d = x_i - x_i, which no position moves
                    const size_t ci = grid.order[j];
                    const SphParticle& cand = particles[ci];
                    float dx, dy, dz, r2, e[3];
                    if (!sph::aggregate_accept(false, false, x[0], x[1], x[2], cand.pos[0], cand.pos[1], cand.pos[2], R2, dx, dy, dz, r2)) continue;
                    if (fluidOnly && cand.isGhost != 0) continue;
                    sph::convgrad_pair_host(bk, R2, dx, dy, dz, r2, gr, values + ci * C, e);
                    if (query) {
                        for (int a = 0; a < 3; ++a) acc[a] = acc[a] - e[a];
                    } else {
                        float b[3];
                        sph::convgrad_pair_host(bk, R2, -dx, -dy, -dz, r2, g + ci * B * C, values + r * C, b);
                        for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (b[a] - e[a]);
                    }
                }
            });
            memcpy((query ? outPoints : outParticles) + r * 3, acc, sizeof(acc));
        }
    }
    if (query && outParticles) {
        const sph::AdjHostRows table(k, points4, m);
        for (size_t r = 0; r < n; ++r) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            sph::adjoint_walk_host(k, stencil, table, particles, points4, r, R2, false, fluidOnly, [&](size_t row, float dx, float dy, float dz, float r2) {
                float e[3];
                sph::convgrad_pair_host(bk, R2, dx, dy, dz, r2, g + row * B * C, values + r * C, e);
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + e[a];
            });
            memcpy(outParticles + r * 3, acc, sizeof(acc));
        }
    }
    return SPH_OK;
}

// ---- state statistics (sph_stats.h) ------------------------------------------------------------------
static int stats_refused(SphEngine* e) {
    if (e->slab) return fail(SPH_ERR_STATE, "statistics of a z-slab engine are not supported: the order of the fp64 sums is defined over one engine's grid");
    return needs_sorted_copy(e, "statistics need");
}

static int stats_check_specs(const SphHistogramSpec* specs, int nSpecs, const uint64_t* histOut, sph::StatK& s) {
    if (nSpecs < 0 || nSpecs > SPH_STAT_MAX_SPECS) return fail(SPH_ERR_ARG, "%d histogram specs (0 .. %d)", nSpecs, (int)SPH_STAT_MAX_SPECS);
    if (nSpecs && (!specs || !histOut)) return fail(SPH_ERR_ARG, "null argument");
    s.nSpecs = nSpecs;
    s.histWords = 0;
    for (int i = 0; i < sph::kStatMaxSpecs; ++i) { s.field[i] = 0; s.bins[i] = 1; s.off[i] = 0; s.lo[i] = 0.0f; s.hi[i] = 1.0f; s.scale[i] = 1.0f; }
    for (int i = 0; i < nSpecs; ++i) {
        const SphHistogramSpec& h = specs[i];
        if (h.field < SPH_STAT_DENSITY || h.field > SPH_STAT_FOAM) return fail(SPH_ERR_ARG, "histogram %d: unknown field %d", i, h.field);
        if (h.bins < 1 || h.bins > SPH_STAT_MAX_BINS) return fail(SPH_ERR_ARG, "histogram %d: %u bins (1 .. %d)", i, h.bins, (int)SPH_STAT_MAX_BINS);
        if (!std::isfinite(h.lo) || !std::isfinite(h.hi)) return fail(SPH_ERR_ARG, "histogram %d: bounds %g, %g are not finite", i, (double)h.lo, (double)h.hi);
        if (!(h.lo < h.hi)) return fail(SPH_ERR_ARG, "histogram %d: lo %g is not below hi %g", i, (double)h.lo, (double)h.hi);
        const float width = h.hi - h.lo;
        const float scale = (float)h.bins / width;
        if (!std::isfinite(width) || !std::isfinite(scale)) return fail(SPH_ERR_ARG, "histogram %d: the bin scale bins / (hi - lo) is not finite in fp32", i);
        s.field[i] = h.field; s.bins[i] = h.bins; s.off[i] = s.histWords; s.lo[i] = h.lo; s.hi[i] = h.hi; s.scale[i] = scale;
        s.histWords += h.bins + 2u;
    }
    return SPH_OK;
}

// Grid build of the current state (as sampling, with order[] for every slot), then tiles, cells, finish and the histogram sum.
static int stats_reduce(SphEngine* e, const sph::StatK& specs, const sph::SimK& k, const float4* pv, const float4* own, const uint32_t* order,
                        const float2* rp, SphStatistics* devOut, uint64_t* devHistOut);
static int stats_run(SphEngine* e, const sph::StatK& specs, SphStatistics* devOut, uint64_t* devHistOut) {
    sph::SimK k;
    int rc;
    if ((rc = sample_grid(e, k, true))) return rc;
    return stats_reduce(e, specs, k, e->d_sPV, e->d_sOwn, e->d_order, e->d_rp[e->cur], devOut, devHistOut);
}
// The reduction over a sorted copy (pv, own), the exact densities rp[order[slot]] and the grid's cellStart (sph_scalars_moments hands it a
// channel laid out as such a copy).
static int stats_reduce(SphEngine* e, const sph::StatK& specs, const sph::SimK& k, const float4* pv, const float4* own, const uint32_t* order,
                        const float2* rp, SphStatistics* devOut, uint64_t* devHistOut) {
    using namespace sph;
    int rc;
    StatK s = specs;
    s.gminx = k.gminx; s.gminy = k.gminy; s.gminz = k.gminz; s.cellSize = k.cellSize;
    s.gx = (float)k.gx; s.gy = (float)k.gy; s.gz = (float)k.gz;
    s.cx = (double)e->params.param_boxCenter[0]; s.cy = (double)e->params.param_boxCenter[1]; s.cz = (double)e->params.param_boxCenter[2];
    s.n = (int)e->n;
    s.numCells = k.numCells;
    s.nTiles = (int)((e->n + kStatTile - 1) / kStatTile);
    s.tilesPow2 = 1;
    while (s.tilesPow2 < s.nTiles) s.tilesPow2 <<= 1;
    s.nBlocks = std::min(s.nTiles, kStatGrid);
    const int cellBlocks = std::min(blocks_for(((size_t)k.numCells + 3) / 4), kStatCellBlocks);
    if ((rc = e->d_statSums.grow(e, (size_t)kStatSums * s.tilesPow2)) ||
        (rc = e->d_statPart.grow(e, (size_t)kStatPartWords * kStatGrid)) ||
        (rc = e->d_statHist.grow(e, (size_t)std::max(s.nBlocks, 1) * std::max(s.histWords, 1u))) ||
        (rc = e->d_statCell.grow(e, (size_t)kStatCellBlocks * kStatCellCols))) return rc;
    if (s.nTiles) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_stats_tiles, dim3(s.nBlocks), dim3(kBlock), 0, e->stream, s, pv, own, order, rp, e->d_statSums.p, e->d_statPart.p, e->d_statHist.p);
    }
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_stats_cells, dim3(cellBlocks), dim3(kBlock), 0, e->stream, (const uint32_t*)e->d_cellStart, k.numCells, e->d_statCell.p);
    }
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_stats_finish, dim3(kStatSums + 2), dim3(kBlock), 0, e->stream, s, e->d_statSums.p, (const uint32_t*)e->d_statPart.p,
                           (const unsigned long long*)e->d_statCell.p, cellBlocks, devOut);
    }
    if (s.histWords) {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_stats_hist, dim3((s.histWords + kStatHistBins - 1u) / kStatHistBins), dim3(kBlock), 0, e->stream, (const uint32_t*)e->d_statHist.p, s.nBlocks, s.histWords,
                           reinterpret_cast<unsigned long long*>(devHistOut));
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_statistics_device(SphEngine* e, SphStatistics* devOut, const SphHistogramSpec* specs, int nSpecs, uint64_t* devHistOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!devOut) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = stats_refused(e))) return rc;
    sph::StatK s{};
    if ((rc = stats_check_specs(specs, nSpecs, devHistOut, s))) return rc;
    return stats_run(e, s, devOut, devHistOut);
}

int sph_statistics(SphEngine* e, SphStatistics* out, const SphHistogramSpec* specs, int nSpecs, uint64_t* histOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = stats_refused(e))) return rc;
    sph::StatK s{};
    if ((rc = stats_check_specs(specs, nSpecs, histOut, s))) return rc;
    const size_t headWords = sizeof(SphStatistics) / sizeof(uint64_t);
    if ((rc = e->d_statOut.grow(e, headWords + (size_t)sph::kStatHistWords))) return rc;
    SphStatistics* devOut = reinterpret_cast<SphStatistics*>(e->d_statOut.p);
    uint64_t* devHist = reinterpret_cast<uint64_t*>(e->d_statOut.p + headWords);
    if ((rc = stats_run(e, s, devOut, devHist))) return rc;
    HIP_TRY(hipMemcpyAsync(out, devOut, sizeof(SphStatistics), hipMemcpyDeviceToHost, e->stream));
    if (s.histWords) HIP_TRY(hipMemcpyAsync(histOut, devHist, (size_t)s.histWords * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

// ---- passive tracers (sph_tracer.h) ---------------------------------------------------------------
static int tracers_check(SphEngine* e, const float* points4, size_t m, int integrator, uint32_t historyCap, uint32_t historyStride) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "tracers on a z-slab engine are not supported: its halo records after a step are the step's entry state");
    if (int rc = needs_sorted_copy(e, "tracers need")) return rc;
    if (m && !points4) return fail(SPH_ERR_ARG, "null argument");
    if (integrator != SPH_TRACER_EULER && integrator != SPH_TRACER_MIDPOINT) return fail(SPH_ERR_ARG, "unknown integrator %d", integrator);
    if (historyStride == 0) return fail(SPH_ERR_ARG, "historyStride must be >= 1");
    if (m > 2147483647ull) return fail(SPH_ERR_ARG, "%zu tracers exceed 2^31 - 1", m);
    if ((unsigned long long)historyCap * (unsigned long long)m > 2147483647ull)
        return fail(SPH_ERR_ARG, "a history of %u snapshots of %zu tracers exceeds 2^31 - 1 float4", historyCap, m);
    return SPH_OK;
}

int sph_tracers_set_device(SphEngine* e, const float* devPoints4, size_t m, int integrator, uint32_t historyCap, uint32_t historyStride) {
    int rc;
    if ((rc = tracers_check(e, devPoints4, m, integrator, historyCap, historyStride))) return rc;
    if (m == 0) { tracers_free(e); return SPH_OK; }
    const size_t ring = (size_t)historyCap * m;
    if (m > e->trCap || ring > e->trRingCap || !e->d_trRec) {             // (a set of the same shape reuses the buffers, and the graphs captured over them)
        tracers_free(e);
        if ((rc = dev_alloc(&e->d_trRec, 2 * m)) || (rc = dev_alloc(&e->d_trPerm, m)) || (rc = dev_alloc(&e->d_trKey, m)) ||
            (rc = dev_alloc(&e->d_trRing, ring)) || (rc = dev_alloc(&e->d_trState, 4))) { tracers_free(e); return rc; }
        e->trCap = m; e->trRingCap = ring;
    }
    e->trM = m; e->trIntegrator = integrator; e->trK = historyCap; e->trS = historyStride;
    e->trSteps = e->trSorted = 0;
    e->trOrdered = false;
    hipLaunchKernelGGL(k_tracer_seed, dim3(blocks_for(m)), dim3(kBlock), 0, e->stream, reinterpret_cast<const float4*>(devPoints4), e->d_trRec, e->d_trPerm,
                       e->d_trRing, e->d_trState, (uint32_t)m, historyCap, historyStride);
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_tracers_set(SphEngine* e, const float* points4, size_t m, int integrator, uint32_t historyCap, uint32_t historyStride) {
    int rc;
    if ((rc = tracers_check(e, points4, m, integrator, historyCap, historyStride))) return rc;
    if (m == 0) { tracers_free(e); return SPH_OK; }
    float4* staging = nullptr;
    if ((rc = dev_alloc(&staging, m))) return rc;
    hipError_t er = hipMemcpyAsync(staging, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream);
    if (er == hipSuccess) rc = sph_tracers_set_device(e, reinterpret_cast<const float*>(staging), m, integrator, historyCap, historyStride);
    const hipError_t es = hipStreamSynchronize(e->stream);
    dev_free(staging);
    if (er != hipSuccess) return fail(SPH_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(er));
    if (rc) return rc;
    if (es != hipSuccess) return fail(SPH_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    return SPH_OK;
}

size_t sph_tracers_count(const SphEngine* e) { return e ? e->trM : 0; }

// The snapshots the pathline ring holds: one per trS substeps, the seed being snapshot 0.
static sph::RingSpan tracers_span(const SphEngine* e) {
    return sph::ring_span((e->trM && e->trK) ? e->trSteps / e->trS + 1 : 0, e->trK);
}
int sph_tracers_info(const SphEngine* e, uint64_t* substeps, uint32_t* snapshots, uint64_t* firstSnapshot) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    const sph::RingSpan span = tracers_span(e);
    if (substeps) *substeps = e->trSteps;
    if (snapshots) *snapshots = span.have;
    if (firstSnapshot) *firstSnapshot = span.first;
    return SPH_OK;
}

int sph_tracers_download(SphEngine* e, SphTracer* out, size_t cap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (cap < e->trM) return fail(SPH_ERR_CAPACITY, "%zu tracers (capacity %zu)", e->trM, cap);
    if (e->trM && !out) return fail(SPH_ERR_ARG, "null argument");
    if (e->trM) HIP_TRY(hipMemcpyAsync(out, e->d_trRec, e->trM * sizeof(SphTracer), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_tracers_device(SphEngine* e, const SphTracer** devPtr) {
    if (!e || !devPtr) return fail(SPH_ERR_ARG, "null argument");
    *devPtr = e->trM ? reinterpret_cast<const SphTracer*>(e->d_trRec) : nullptr;
    return SPH_OK;
}

int sph_tracers_history(SphEngine* e, float* out4, size_t snapshotCap, uint32_t* snapshotsOut, uint64_t* firstSnapshotOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->trM || !e->trK) return fail(SPH_ERR_STATE, "no pathline history: call sph_tracers_set with historyCap >= 1 first");
    const sph::RingSpan span = tracers_span(e);
    if (snapshotCap < span.have) return fail(SPH_ERR_CAPACITY, "%u snapshots (capacity %zu)", span.have, snapshotCap);
    if (!out4) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = ring_read(e, e->d_trRing, e->trM * sizeof(float4), e->trK, span, out4))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (snapshotsOut) *snapshotsOut = span.have;
    if (firstSnapshotOut) *firstSnapshotOut = span.first;
    return SPH_OK;
}

// ---- spray, foam and bubbles (sph_diffuse.h) ------------------------------------------------------
static bool diffuse_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }
static int diffuse_check_config(const SphDiffuseConfig& c) {
    if (!diffuse_nonneg(c.rate) || !diffuse_nonneg(c.lifeMin) || !diffuse_nonneg(c.lifeMax) || !diffuse_nonneg(c.spread))
        return fail(SPH_ERR_ARG, "diffuse rate, lifeMin, lifeMax and spread must be finite and >= 0");
    if (c.lifeMax < c.lifeMin) return fail(SPH_ERR_ARG, "diffuse lifeMax %g < lifeMin %g", (double)c.lifeMax, (double)c.lifeMin);
    if (c.maxPerParent < 1u || c.maxPerParent > 8u) return fail(SPH_ERR_ARG, "diffuse maxPerParent %u (1 .. 8)", c.maxPerParent);
    if (c.sprayBelow > c.bubbleAbove) return fail(SPH_ERR_ARG, "diffuse sprayBelow %u > bubbleAbove %u", c.sprayBelow, c.bubbleAbove);
    if (!(c.kd >= 0.0f && c.kd <= 1.0f)) return fail(SPH_ERR_ARG, "diffuse kd %g outside [0, 1]", (double)c.kd);
    if (!std::isfinite(c.threshold) || !std::isfinite(c.kb)) return fail(SPH_ERR_ARG, "diffuse threshold and kb must be finite");
    if (!(c.maxAge >= 0.0f)) return fail(SPH_ERR_ARG, "diffuse maxAge must be >= 0");
    if (c.capacity > 2147483647u) return fail(SPH_ERR_ARG, "a diffuse capacity of %u exceeds 2^31 - 1", c.capacity);
    return SPH_OK;
}
static sph::DiffuseCoef diffuse_coef_of(const SphDiffuseConfig& c) {
    return sph::DiffuseCoef{c.threshold, c.rate, c.lifeMin, c.lifeMax, c.spread, c.kb, c.kd, c.maxAge, c.sprayBelow, c.bubbleAbove, c.maxPerParent, c.seed};
}
void sph_diffuse_default(SphDiffuseConfig* out) {
    if (!out) return;
    SphDiffuseConfig c{};
    c.capacity = 65536u; c.seed = 1u;
    c.threshold = 0.02f; c.rate = 5000.0f;
    c.lifeMin = 0.2f; c.lifeMax = 1.0f;
    c.spread = 0.5f; c.maxAge = 4.0f;
    c.sprayBelow = 6u; c.bubbleAbove = 20u;
    c.kb = 2.0f; c.kd = 0.5f;
    c.maxPerParent = 4u;
    *out = c;
}
int sph_diffuse_set(SphEngine* e, const SphDiffuseConfig* cfg) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "diffuse particles on a z-slab engine are not supported: a record would have to migrate with the fluid around it");
    int rc;
    if ((rc = needs_sorted_copy(e, "diffuse particles need"))) return rc;
    if (!cfg || cfg->capacity == 0u) { diffuse_free(e); return SPH_OK; }
    if ((rc = diffuse_check_config(*cfg))) return rc;
    const uint32_t C = cfg->capacity;
    if (C != e->dfC || !e->d_dfPool) {
        diffuse_free(e);
        const size_t cb = (size_t)blocks_for((size_t)C);
        if ((rc = dev_alloc(&e->d_dfPool, (size_t)3 * C)) || (rc = dev_alloc(&e->d_dfScratch, (size_t)3 * C)) || (rc = dev_alloc(&e->d_dfState, (size_t)DF_WORDS)) ||
            (rc = e->d_dfCoef.ensure(e, 1, "pinned staging of the diffuse coefficients")) || (rc = dev_alloc(&e->d_dfFlag, (size_t)C + 8)) ||
            (rc = dev_alloc(&e->d_dfFlagStart, (size_t)C + 1)) || (rc = dev_alloc(&e->d_dfFlagSums, (size_t)blocks_for((size_t)C, kScanTile) + 1)) ||
            (rc = dev_alloc(&e->d_dfPart, cb * DF_PART_WORDS))) {
            diffuse_free(e);
            return rc;
        }
        hipError_t m1 = hipMemsetAsync(e->d_dfState, 0, DF_WORDS * sizeof(uint32_t), e->stream);
        hipError_t m2 = hipMemsetAsync(e->d_dfFlag, 0, ((size_t)C + 8) * sizeof(uint32_t), e->stream);    // (k_scan_apply leaves it zero again)
        if (m1 != hipSuccess || m2 != hipSuccess) { diffuse_free(e); return fail(SPH_ERR_HIP, "hipMemsetAsync of the diffuse pool failed"); }
        e->dfC = C;
    }
    const sph::DiffuseCoef coef = diffuse_coef_of(*cfg);
    if ((rc = e->d_dfCoef.put(e, &coef))) return rc;
    e->dfCfg = *cfg;
    return SPH_OK;
}
int sph_diffuse_get(SphEngine* e, SphDiffuseConfig* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->dfCfg;
    return SPH_OK;
}
static void diffuse_info_of(const uint32_t* w, uint32_t C, SphDiffuseInfo& o) {
    auto u64 = [&](int i) { return ((uint64_t)w[i + 1] << 32) | w[i]; };
    o = SphDiffuseInfo{};
    o.substeps = u64(DF_STEP_LO);
    o.spawned = u64(DF_TOTALS); o.dropped = u64(DF_TOTALS + 2); o.diedLife = u64(DF_TOTALS + 4); o.diedAge = u64(DF_TOTALS + 6);
    o.leftBox = u64(DF_TOTALS + 8); o.nonFinite = u64(DF_TOTALS + 10); o.seeded = u64(DF_TOTALS + 12);
    o.alive = std::min(w[DF_ALIVE], C); o.capacity = C;
    for (int q = 0; q < 3; ++q) o.aliveByKind[q] = w[DF_CLASS + q];
}
int sph_diffuse_info(SphEngine* e, SphDiffuseInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = SphDiffuseInfo{};
    if (!e->dfC) return SPH_OK;
    uint32_t w[DF_WORDS];
    HIP_TRY(hipMemcpyAsync(w, e->d_dfState, sizeof(w), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    diffuse_info_of(w, e->dfC, *out);
    return SPH_OK;
}
int sph_diffuse_download(SphEngine* e, SphDiffuse* out, size_t cap, size_t* countOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    SphDiffuseInfo info;
    int rc;
    if ((rc = sph_diffuse_info(e, &info))) return rc;
    if (cap < info.alive) return fail(SPH_ERR_CAPACITY, "%u diffuse particles (capacity %zu)", info.alive, cap);
    if (info.alive && !out) return fail(SPH_ERR_ARG, "null argument");
    if (info.alive) {
        HIP_TRY(hipMemcpyAsync(out, e->d_dfPool, (size_t)info.alive * sizeof(SphDiffuse), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (countOut) *countOut = info.alive;
    return SPH_OK;
}
int sph_diffuse_device(SphEngine* e, const SphDiffuse** records, const uint32_t** aliveCountWord) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (records) *records = e->dfC ? reinterpret_cast<const SphDiffuse*>(e->d_dfPool) : nullptr;
    if (aliveCountWord) *aliveCountWord = e->dfC ? e->d_dfState + DF_ALIVE : nullptr;
    return SPH_OK;
}
int sph_diffuse_seed(SphEngine* e, const SphDiffuse* records, size_t m) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->dfC) return fail(SPH_ERR_STATE, "no diffuse pool: call sph_diffuse_set first");
    if (m == 0) return SPH_OK;
    if (!records) return fail(SPH_ERR_ARG, "null argument");
    uint32_t w[DF_WORDS];
    HIP_TRY(hipMemcpyAsync(w, e->d_dfState, sizeof(w), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const uint32_t alive = std::min(w[DF_ALIVE], e->dfC);
    if (m > (size_t)(e->dfC - alive)) return fail(SPH_ERR_CAPACITY, "%zu diffuse records behind %u living ones exceed the capacity of %u", m, alive, e->dfC);
    for (size_t i = 0; i < m; ++i) if (records[i].kind <= 2u) w[DF_CLASS + records[i].kind] += 1u;
    w[DF_ALIVE] = alive + (uint32_t)m;
    const uint64_t seeded = (((uint64_t)w[DF_TOTALS + 13] << 32) | w[DF_TOTALS + 12]) + m;
    w[DF_TOTALS + 12] = (uint32_t)seeded; w[DF_TOTALS + 13] = (uint32_t)(seeded >> 32);
    HIP_TRY(hipMemcpy(e->d_dfPool + (size_t)3 * alive, records, m * sizeof(SphDiffuse), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_dfState, w, sizeof(w), hipMemcpyHostToDevice));
    return SPH_OK;
}
// ---- crest births of the pool ----
static_assert(sizeof(SphDiffuseCrest) == 48 && sizeof(SphDiffuseCrestInfo) == 32 && sizeof(sph::DiffuseCrestCoef) == 32, "SphDiffuseCrest is 48 bytes, SphDiffuseCrestInfo 32");
static bool crest_window(float lo, float hi) { return std::isfinite(lo) && std::isfinite(hi) && lo < hi; }
// The crest config as an argument (h and cellSize: of the params the shell pass would run with).
static int diffuse_check_crest(const SphDiffuseCrest& c, float h, float cellSize) {
    if (!diffuse_nonneg(c.rate)) return fail(SPH_ERR_ARG, "diffuse crest rate must be finite and >= 0");
    float radius = 0.0f;
    int stencil = 0, rc;
    if (!std::isfinite(c.radius)) return fail(SPH_ERR_ARG, "diffuse crest radius %g is not finite", (double)c.radius);
    if ((rc = shell_check(diffuse_crest_shell_config(c), h, cellSize, &radius, &stencil))) return rc;
    if (!crest_window(c.crestMin, c.crestMax)) return fail(SPH_ERR_ARG, "diffuse crest window [%g, %g] is empty or not finite", (double)c.crestMin, (double)c.crestMax);
    if (!crest_window(c.speedMin, c.speedMax)) return fail(SPH_ERR_ARG, "diffuse crest speed window [%g, %g] is empty or not finite", (double)c.speedMin, (double)c.speedMax);
    if (!(c.align >= 0.0f && c.align <= 1.0f)) return fail(SPH_ERR_ARG, "diffuse crest align %g outside [0, 1]", (double)c.align);
    if (c.every == 0u) return fail(SPH_ERR_ARG, "diffuse crest every must be >= 1");
    return SPH_OK;
}
static sph::DiffuseCrestCoef diffuse_crest_coef_of(const SphDiffuseCrest& c) {
    return sph::DiffuseCrestCoef{c.rate, c.crestMin, c.crestMax, c.speedMin, c.speedMax, c.align, c.every, 0u};
}
void sph_diffuse_crest_default(SphDiffuseCrest* out) {
    if (!out) return;
    SphDiffuseCrest c{};
    c.rate = 300.0f; c.radius = 0.0f; c.offset = 0.10f; c.minCount = 0u; c.flags = 0;
    c.crestMin = 0.5f; c.crestMax = 2.0f;
    c.speedMin = 20.0f; c.speedMax = 60.0f;
    c.align = 0.6f; c.every = 1u;
    *out = c;
}
int sph_diffuse_set_crest(SphEngine* e, const SphDiffuseCrest* crest) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->dfC) return fail(SPH_ERR_STATE, "no diffuse pool: call sph_diffuse_set first");
    if (!crest || crest->rate == 0.0f) {                                // off: the launches of before; the books stay
        e->dfCrOn = false;
        e->dfCrCfg = SphDiffuseCrest{};
        return SPH_OK;
    }
    int rc;
    if ((rc = validate_params(e->params))) return rc;
    SphGridInfo g;
    sph::compute_grid_extents(e->params, g);
    if ((rc = diffuse_check_crest(*crest, e->params.param_h, g.cellSize))) return rc;
    if (!e->d_dfCrCoef.p) {
        hipError_t er = hipSuccess;
        if ((rc = e->d_dfCrCoef.ensure(e, 1, "staging of the diffuse crest coefficients")) || (rc = dev_alloc(&e->d_dfCrState, (size_t)DFC_WORDS)) ||
            (er = hipMemsetAsync(e->d_dfCrState, 0, DFC_WORDS * sizeof(uint32_t), e->stream)) != hipSuccess) {
            HIP_TRY(hipStreamSynchronize(e->stream));                  // (a memset may have been queued)
            diffuse_crest_free(e);
            return rc ? rc : fail(SPH_ERR_HIP, "staging of the diffuse crest coefficients: %s", hipGetErrorString(er));
        }
    }
    const sph::DiffuseCrestCoef coef = diffuse_crest_coef_of(*crest);
    if ((rc = e->d_dfCrCoef.put(e, &coef))) return rc;
    e->dfCrCfg = *crest;
    e->dfCrCfg.pad = 0u;
    e->dfCrOn = true;
    return SPH_OK;
}
int sph_diffuse_get_crest(SphEngine* e, SphDiffuseCrest* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = e->dfCrCfg;
    return SPH_OK;
}
int sph_diffuse_crest_info(SphEngine* e, SphDiffuseCrestInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    *out = SphDiffuseCrestInfo{};
    if (!e->dfC || !e->d_dfCrState) return SPH_OK;
    uint32_t w[DFC_WORDS];
    HIP_TRY(hipMemcpyAsync(w, e->d_dfCrState, sizeof(w), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    out->acting = ((uint64_t)w[DFC_ACTING + 1] << 32) | w[DFC_ACTING];
    out->crestSpawned = ((uint64_t)w[DFC_SPAWNED + 1] << 32) | w[DFC_SPAWNED];
    out->shellSize = w[DFC_SHELL];
    out->on = e->dfCrOn ? 1 : 0;
    if (e->dfCrOn && validate_params(e->params) == SPH_OK) {
        SphGridInfo g;
        sph::compute_grid_extents(e->params, g);
        (void)diffuse_crest_args(e, g.cellSize, &out->radius, &out->stencil);
    }
    return SPH_OK;
}

static int diffuse_step_host_run(const SphDiffuseConfig* cfg, const SphDiffuseCrest* crest, const SphParams* params, float dt, uint64_t substep,
                                 const SphDiffuse* pool, size_t m, const SphSample* samples, const SphParticle* particles, size_t n,
                                 const SphShell* shellRows, SphDiffuse* out, size_t* countOut, SphDiffuseInfo* totals, SphDiffuseCrestInfo* crestTotals) {
    if (!cfg || !params || !countOut || (m && (!pool || !samples)) || (n && !particles)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = diffuse_check_config(*cfg)) || (rc = validate_params(*params))) return rc;
    if (crest) {
        SphGridInfo cg;
        sph::compute_grid_extents(*params, cg);
        if ((rc = diffuse_check_crest(*crest, params->param_h, cg.cellSize))) return rc;
        if (n && !shellRows) return fail(SPH_ERR_ARG, "null argument");
    }
    const size_t C = cfg->capacity;
    if (m > C) return fail(SPH_ERR_CAPACITY, "%zu diffuse records exceed the capacity of %zu", m, C);
    if (C && !out) return fail(SPH_ERR_ARG, "null argument");
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    if (params->param_pause) {
        if (out != pool && m) std::memmove(out, pool, m * sizeof(SphDiffuse));
        *countOut = m;
        return SPH_OK;
    }
    const float step = dt > 0.0f ? dt : params->param_timeStep;
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, step, k);
    const float gmin[3] = {k.gminx, k.gminy, k.gminz};
    const int dims[3] = {k.gx, k.gy, k.gz};
    const sph::DiffuseBox box = sph::diffuse_box(gmin, k.cellSize, dims, k.gravx, k.gravy, k.gravz);
    const sph::DiffuseCoef co = diffuse_coef_of(*cfg);
    const uint32_t lo = (uint32_t)substep, hi = (uint32_t)(substep >> 32);
    uint64_t died[5] = {0, 0, 0, 0, 0};
    uint32_t kinds[3] = {0, 0, 0};
    std::vector<SphDiffuse> next;
    next.reserve(m);
    for (size_t i = 0; i < m; ++i) {                                   // 1. advance, 3. the survivors in their order
        sph::DiffuseRec r;
        std::memcpy(&r, &pool[i], sizeof(r));
        const SphSample& s = samples[i];
        const int fate = sph::diffuse_move(co, box, step, s.vel[0], s.vel[1], s.vel[2], s.count, r);
        died[fate] += 1;
        if (fate != sph::DF_LIVES) continue;
        SphDiffuse o;
        std::memcpy(&o, &r, sizeof(o));
        next.push_back(o);
        kinds[r.kind] += 1u;
    }
    const size_t survivors = next.size();
    uint64_t spawned = 0, crestSpawned = 0;
    uint32_t shellSize = 0;
    const sph::DiffuseCrestCoef cc = crest ? diffuse_crest_coef_of(*crest) : sph::DiffuseCrestCoef{};
    const bool acts = crest && sph::diffuse_crest_acts(lo, hi, cc.every);
    for (size_t i = 0; i < n; ++i) {                                   // 2. spawn, in id order
        const SphParticle& p = particles[i];
        const uint32_t flags = (p.isGhost == 1 ? F_GHOST1 : 0u) | (p.isGhost != 0 ? F_GHOSTNZ : 0u) | (p.isActive == 0 ? F_INACTIVE : 0u);
        const float invRho = p.density > 0.0f ? 1.0f / p.density : 0.0f;
        uint32_t children = sph::diffuse_children(co, step, p.padA, flags, invRho, (uint32_t)i, lo, hi);
        if (acts) {                                                    // the crest term's children behind the foam term's
            const SphShell& s = shellRows[i];
            const bool member = (s.flags & SPH_SHELL_MEMBER) != 0;
            if (member) shellSize += 1u;
            const uint32_t born = sph::diffuse_crest_children(co, cc, step, flags, invRho, member, (s.flags & SPH_SHELL_ISOLATED) != 0, s.normal[0],
                                                              s.normal[1], s.normal[2], s.crest, p.vel[0], p.vel[1], p.vel[2], (uint32_t)i, lo, hi);
            const uint32_t all = std::min(children + born, co.maxPerParent);
            crestSpawned += all - children;
            children = all;
        }
        for (uint32_t q = 0; q < children; ++q) {
            if (next.size() < C) {
                const sph::DiffuseRec r = sph::diffuse_child(co, k.h, p.pos[0], p.pos[1], p.pos[2], p.vel[0], p.vel[1], p.vel[2], (uint32_t)i, lo, hi, q);
                SphDiffuse o;
                std::memcpy(&o, &r, sizeof(o));
                next.push_back(o);
            }
        }
        spawned += children;
    }
    const uint64_t born = next.size() - survivors;
    if (!next.empty()) std::memcpy(out, next.data(), next.size() * sizeof(SphDiffuse));
    *countOut = next.size();
    if (totals) {
        totals->substeps += 1;
        totals->spawned += spawned; totals->dropped += spawned - born;
        totals->diedLife += died[sph::DF_DIED_LIFE]; totals->diedAge += died[sph::DF_DIED_AGE];
        totals->leftBox += died[sph::DF_DIED_BOX]; totals->nonFinite += died[sph::DF_DIED_NONFINITE];
        totals->alive = (uint32_t)next.size(); totals->capacity = (uint32_t)C;
        totals->aliveByKind[0] = kinds[0]; totals->aliveByKind[1] = kinds[1] + (uint32_t)born; totals->aliveByKind[2] = kinds[2];
    }
    if (crestTotals && acts) {
        crestTotals->acting += 1;
        crestTotals->crestSpawned += crestSpawned;
        crestTotals->shellSize = shellSize;
    }
    return SPH_OK;
}
int sph_diffuse_step_host(const SphDiffuseConfig* cfg, const SphParams* params, float dt, uint64_t substep, const SphDiffuse* pool, size_t m,
                          const SphSample* samples, const SphParticle* particles, size_t n, SphDiffuse* out, size_t* countOut, SphDiffuseInfo* totals) {
    return diffuse_step_host_run(cfg, nullptr, params, dt, substep, pool, m, samples, particles, n, nullptr, out, countOut, totals, nullptr);
}
int sph_diffuse_step_host_crest(const SphDiffuseConfig* cfg, const SphDiffuseCrest* crest, const SphParams* params, float dt, uint64_t substep,
                                const SphDiffuse* pool, size_t m, const SphSample* samples, const SphParticle* particles, size_t n,
                                const SphShell* shellRows, SphDiffuse* out, size_t* countOut, SphDiffuseInfo* totals, SphDiffuseCrestInfo* crestTotals) {
    const bool on = crest && crest->rate != 0.0f;                      // (NULL or rate == 0: sph_diffuse_step_host)
    return diffuse_step_host_run(cfg, on ? crest : nullptr, params, dt, substep, pool, m, samples, particles, n, shellRows, out, countOut, totals,
                                 on ? crestTotals : nullptr);
}

// ---- diffusing scalars (sph_scalar.h) -------------------------------------------------------------
static int scalars_refused(SphEngine* e) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "scalars on a z-slab engine are not supported: halo records would have to carry them");
    return needs_sorted_copy(e, "scalars need");
}
static int scalars_check_coeffs(const float* coeffs, int K) {
    if (!coeffs) return fail(SPH_ERR_ARG, "null argument");
    for (int i = 0; i < 2 * K; ++i)
        if (!std::isfinite(coeffs[i]) || coeffs[i] < 0.0f)
            return fail(SPH_ERR_ARG, "%s %d is %g (must be finite and >= 0)", i < K ? "diffusivity" : "decay rate", i % K, (double)coeffs[i]);
    return SPH_OK;
}
// The coefficients as set, through a pinned slot, to the device record the kernels read: stream-ordered.
static int scalars_upload_coef(SphEngine* e) {
    sph::ScalarCoef* slot = nullptr;
    int rc;
    if ((rc = e->d_scCoef.slot(&slot))) return rc;
    sph::scalar_make_coef(e->scK, e->scCoeffs, *slot);
    return e->d_scCoef.send(e);
}
static int scalars_check_set(SphEngine* e, size_t n, int channels, const float* coeffs) {
    int rc;
    if ((rc = scalars_refused(e))) return rc;
    if (channels == 0) return SPH_OK;
    if (channels < 1 || channels > SPH_MAX_SCALAR_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (1 .. %d)", channels, SPH_MAX_SCALAR_CHANNELS);
    if (n != e->n) return fail(SPH_ERR_ARG, "%zu values per channel for an engine of %zu particles", n, e->n);
    return scalars_check_coeffs(coeffs, channels);
}

static int couple_clear(SphEngine* e);

int sph_scalars_set_device(SphEngine* e, const float* devValues, size_t n, int channels, const float* coeffs) {
    int rc;
    if ((rc = scalars_check_set(e, n, channels, coeffs))) return rc;
    if (channels == 0) { scalars_free(e); return SPH_OK; }
    if (channels != e->scK || n != e->scN || !e->d_scVal) {              // (a set of the same shape reuses the buffers, and the graphs captured over them)
        scalars_free(e);
        if ((rc = dev_alloc(&e->d_scVal, n * (size_t)channels)) || (rc = dev_alloc(&e->d_scSorted, n * (size_t)(channels + 1))) ||
            (rc = e->d_scCoef.ensure(e, 1, "pinned staging of the scalar coefficients")) || (rc = dev_alloc(&e->d_scState, 4))) {
            scalars_free(e);
            return rc;
        }
        e->scN = n;
    }
    e->scK = channels;
    e->scSteps = 0;
    std::memcpy(e->scCoeffs, coeffs, sizeof(float) * 2 * (size_t)channels);
    if ((rc = scalars_upload_coef(e)) || (rc = couple_clear(e))) return rc;   // (a new set starts without buoyancy and without sources)
    if (devValues) {
        if (n) HIP_TRY(hipMemcpyAsync(e->d_scVal, devValues, n * (size_t)channels * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
        hipLaunchKernelGGL(k_scalar_clear_state, dim3(1), dim3(64), 0, e->stream, e->d_scState);
    } else {
        // channel 0 = padB of the records (never rewritten by a substep, so the 80-byte array holds it whether or not it is current)
        hipLaunchKernelGGL(k_scalar_seed, dim3(std::max(1, blocks_for(n))), dim3(kBlock), 0, e->stream, (const SphParticle*)e->d_aos, e->d_scVal, e->d_scState,
                           channels, (uint32_t)n);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_scalars_set(SphEngine* e, const float* values, size_t n, int channels, const float* coeffs) {
    int rc;
    if ((rc = scalars_check_set(e, n, channels, coeffs))) return rc;
    if (channels == 0) { scalars_free(e); return SPH_OK; }
    float* staging = nullptr;
    hipError_t er = hipSuccess;
    if (values) {
        if ((rc = dev_alloc(&staging, n * (size_t)channels))) return rc;
        if (n) er = hipMemcpyAsync(staging, values, n * (size_t)channels * sizeof(float), hipMemcpyHostToDevice, e->stream);
    }
    if (er == hipSuccess) rc = sph_scalars_set_device(e, staging, n, channels, coeffs);
    const hipError_t es = hipStreamSynchronize(e->stream);
    dev_free(staging);
    if (er != hipSuccess) return fail(SPH_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(er));
    if (rc) return rc;
    if (es != hipSuccess) return fail(SPH_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    return SPH_OK;
}

int sph_scalars_set_coefficients(SphEngine* e, const float* coeffs) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    int rc;
    if ((rc = scalars_check_coeffs(coeffs, e->scK))) return rc;
    std::memcpy(e->scCoeffs, coeffs, sizeof(float) * 2 * (size_t)e->scK);
    return scalars_upload_coef(e);
}

int sph_scalars_channels(const SphEngine* e) { return e ? e->scK : 0; }

int sph_scalars_download(SphEngine* e, float* out, size_t cap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    const size_t total = e->scK ? e->scN * (size_t)e->scK : 0;
    if (cap < total) return fail(SPH_ERR_CAPACITY, "%zu values (capacity %zu)", total, cap);
    if (total && !out) return fail(SPH_ERR_ARG, "null argument");
    if (total) HIP_TRY(hipMemcpyAsync(out, e->d_scVal, total * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_scalars_device(SphEngine* e, const float** devPtr) {
    if (!e || !devPtr) return fail(SPH_ERR_ARG, "null argument");
    *devPtr = e->scK ? e->d_scVal : nullptr;
    return SPH_OK;
}

int sph_scalars_paint(SphEngine* e, const float center[3], float radius, int channel, float value, int mode) {
    if (!e || !center) return fail(SPH_ERR_ARG, "null argument");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    if (channel < 0 || channel >= e->scK) return fail(SPH_ERR_ARG, "channel %d of %d", channel, e->scK);
    if (mode != SPH_SCALAR_SET && mode != SPH_SCALAR_ADD) return fail(SPH_ERR_ARG, "unknown mode %d", mode);
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(SPH_ERR_ARG, "radius %g (must be finite and > 0)", (double)radius);
    if (!e->internalValid && !e->aosValid) return fail(SPH_ERR_STATE, "no valid particle state");
    if (e->n) {
        // the engine's own state arrays while they hold the state, else the 80-byte records (after an upload): nothing is materialised
        const bool own = e->internalValid;
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_scalar_paint, dim3(blocks_for(e->n)), dim3(kBlock), 0, e->stream, own ? (const float4*)e->d_pos[e->cur] : (const float4*)nullptr,
                           (const float4*)e->d_vel[e->cur], (const SphParticle*)e->d_aos, e->d_scVal, e->scK, channel, center[0], center[1], center[2],
                           radius * radius, value, mode, e->idBase, (uint32_t)e->n);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_scalars_info(SphEngine* e, uint64_t* substepsOut, float* maxNumberOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (substepsOut) *substepsOut = e->scK ? e->scSteps : 0;
    if (maxNumberOut) {
        *maxNumberOut = 0.0f;
        if (e->scK) {
            HIP_TRY(hipMemcpyAsync(maxNumberOut, e->d_scState, sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
    }
    return SPH_OK;
}

// Grid of the CURRENT state (as sampling builds it) and the values gathered into its slot order; the diffusion number is left alone.
static int scalars_sample_grid(SphEngine* e, int channel, SimK& k, bool orderAll = false) {
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    if (channel < 0 || channel >= e->scK) return fail(SPH_ERR_ARG, "channel %d of %d", channel, e->scK);
    int rc;
    if ((rc = sample_grid(e, k, orderAll))) return rc;
    const uint32_t n = (uint32_t)e->n;
    if (n) {
        Timed t(e, SPH_K_OTHER);
        scalars_gather_now(e, n);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_scalars_moments(SphEngine* e, SphScalarMoments* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    int rc;
    if ((rc = stats_refused(e))) return rc;
    SimK k;
    if ((rc = sample_grid(e, k, true))) return rc;
    const size_t n = e->n, headWords = sizeof(SphStatistics) / sizeof(uint64_t);
    if ((rc = e->d_scView.grow(e, 3 * n)) || (rc = e->d_scViewRp.grow(e, n)) || (rc = e->d_statOut.grow(e, headWords * (size_t)sph::kScalarMax + (size_t)sph::kStatHistWords)))
        return rc;
    sph::StatK s{};
    if ((rc = stats_check_specs(nullptr, 0, nullptr, s))) return rc;
    float4* vPv = e->d_scView.p;
    float4* vOwn = e->d_scView.p + 2 * n;
    for (int c = 0; c < e->scK; ++c) {
        if (n) {
            Timed t(e, SPH_K_OTHER);
            hipLaunchKernelGGL(k_scalar_stat_view, dim3(blocks_for(n)), dim3(kBlock), 0, e->stream, (const float4*)e->d_sPV, (const float4*)e->d_sOwn,
                               (const uint32_t*)e->d_order, (const float*)e->d_scVal, e->scK, c, vPv, vOwn, e->d_scViewRp.p, e->idBase, (uint32_t)n);
        }
        if ((rc = stats_reduce(e, s, k, vPv, vOwn, e->d_order, e->d_scViewRp.p, reinterpret_cast<SphStatistics*>(e->d_statOut.p + headWords * (size_t)c), nullptr)))
            return rc;
    }
    std::vector<SphStatistics> st((size_t)e->scK);
    HIP_TRY(hipMemcpyAsync(st.data(), e->d_statOut.p, sizeof(SphStatistics) * (size_t)e->scK, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int c = 0; c < e->scK; ++c) {
        out[c].count = st[c].numCounted;
        out[c].sum = st[c].sumPos[0];
        out[c].sumSquares = st[c].sumDensity2;
        out[c].min = st[c].minPos[0];
        out[c].max = st[c].maxPos[0];
    }
    return SPH_OK;
}

int sph_scalars_sample_points_device(SphEngine* e, const float* devPoints4, size_t m, int channel, float* devOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (m && (!devPoints4 || !devOut)) return fail(SPH_ERR_ARG, "null argument");
    if (m > (size_t)1 << 40) return fail(SPH_ERR_ARG, "%zu probes", m);
    SimK k;
    int rc;
    if ((rc = scalars_sample_grid(e, channel, k))) return rc;
    if (m) {
        Timed t(e, SPH_K_OTHER);
        const float4* pts = reinterpret_cast<const float4*>(devPoints4);
        const dim3 grid(blocks_for(m)), block(kBlock);
        switch (e->scK) {
        case 1: hipLaunchKernelGGL((k_scalar_sample_points<1>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, pts, devOut, m); break;
        case 2: hipLaunchKernelGGL((k_scalar_sample_points<2>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, pts, devOut, m); break;
        case 3: hipLaunchKernelGGL((k_scalar_sample_points<3>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, pts, devOut, m); break;
        default: hipLaunchKernelGGL((k_scalar_sample_points<4>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, pts, devOut, m); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_scalars_sample_points(SphEngine* e, const float* points4, size_t m, int channel, float* out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (m && (!points4 || !out)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = scalars_refused(e))) return rc;
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    if (channel < 0 || channel >= e->scK) return fail(SPH_ERR_ARG, "channel %d of %d", channel, e->scK);
    if (m && ((rc = e->d_sampleIn.grow(e, m)) || (rc = e->d_scSampleOut.grow(e, m)))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(e->d_sampleIn.p, points4, m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    if ((rc = sph_scalars_sample_points_device(e, reinterpret_cast<const float*>(e->d_sampleIn.p), m, channel, e->d_scSampleOut.p))) return rc;
    if (m) HIP_TRY(hipMemcpyAsync(out, e->d_scSampleOut.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_scalars_sample_lattice(SphEngine* e, const float origin[3], const float spacing[3], const int dims[3], int channel, float* devOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!origin || !spacing || !dims || !devOut) return fail(SPH_ERR_ARG, "null argument");
    SimK k;
    int rc;
    long long total = 0;
    if ((rc = check_lattice(dims, spacing, 1, &total)) || (rc = scalars_sample_grid(e, channel, k))) return rc;
    {
        Timed t(e, SPH_K_OTHER);
        const dim3 grid((unsigned)std::min<long long>((total + kBlock - 1) / kBlock, 1ll << 20)), block(kBlock);
        switch (e->scK) {
        case 1: hipLaunchKernelGGL((k_scalar_sample_lattice<1>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2], dims[0], dims[1], total, devOut); break;
        case 2: hipLaunchKernelGGL((k_scalar_sample_lattice<2>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2], dims[0], dims[1], total, devOut); break;
        case 3: hipLaunchKernelGGL((k_scalar_sample_lattice<3>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2], dims[0], dims[1], total, devOut); break;
        default: hipLaunchKernelGGL((k_scalar_sample_lattice<4>), grid, block, 0, e->stream, k, (const float4*)e->d_sPV, (const uint32_t*)e->d_cellStart, (const float*)e->d_scSorted, channel, origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2], dims[0], dims[1], total, devOut); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_scalars_step_host(const SphParticle* particles, size_t n, const SphParams* params, float dt, float* values, int channels, const float* coeffs,
                          float* maxNumberOut) {
    if (!params || (n && (!particles || !values))) return fail(SPH_ERR_ARG, "null argument");
    if (channels < 1 || channels > SPH_MAX_SCALAR_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (1 .. %d)", channels, SPH_MAX_SCALAR_CHANNELS);
    int rc;
    if ((rc = scalars_check_coeffs(coeffs, channels)) || (rc = validate_params(*params))) return rc;
    if (n > kMaxParticles) return fail(SPH_ERR_CAPACITY, "%zu particles exceed the engine limit of %zu", n, kMaxParticles);
    const float step = dt > 0.0f ? dt : params->param_timeStep;
    SphGridInfo g;
    sph::compute_grid_extents(*params, g);
    SimK k;
    sph::make_simk(*params, g, step, k);
    sph::ScalarCoef co;
    sph::scalar_make_coef(channels, coeffs, co);
    const float kLap = sph::scalar_klap(params->param_mass, params->param_h);
    float mx = 0.0f;
    if (!params->param_pause) {
        switch (channels) {
        case 1: mx = scalars_step_loop<1>(k, kLap, step, co, particles, n, values); break;
        case 2: mx = scalars_step_loop<2>(k, kLap, step, co, particles, n, values); break;
        case 3: mx = scalars_step_loop<3>(k, kLap, step, co, particles, n, values); break;
        default: mx = scalars_step_loop<4>(k, kLap, step, co, particles, n, values); break;
        }
    }
    if (maxNumberOut) *maxNumberOut = mx;
    return SPH_OK;
}

// ---- kinematic solid obstacles (sph_obstacle.h) --------------------------------------------------
static bool obs_all_finite(const float* v, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}
static int obstacles_check(const SphObstacle* obs, int count) {
    if (count < 0 || count > SPH_MAX_OBSTACLES) return fail(SPH_ERR_ARG, "obstacle count %d outside 0..%d", count, SPH_MAX_OBSTACLES);
    if (count && !obs) return fail(SPH_ERR_ARG, "null argument");
    for (int i = 0; i < count; ++i) {
        const SphObstacle& o = obs[i];
        if (o.shape != SPH_OBSTACLE_SPHERE && o.shape != SPH_OBSTACLE_BOX && o.shape != SPH_OBSTACLE_CAPSULE) return fail(SPH_ERR_ARG, "obstacle %d: unknown shape %d", i, o.shape);
        if (!obs_all_finite(o.size, 3) || !obs_all_finite(o.center, 3) || !obs_all_finite(o.rotation, 4) || !obs_all_finite(o.vel, 3) ||
            !obs_all_finite(o.omega, 3) || !std::isfinite(o.restitution) || !std::isfinite(o.friction))
            return fail(SPH_ERR_ARG, "obstacle %d: a field is not finite", i);
        const int used = o.shape == SPH_OBSTACLE_SPHERE ? 1 : (o.shape == SPH_OBSTACLE_CAPSULE ? 2 : 3);
        for (int a = 0; a < used; ++a) if (!(o.size[a] > 0.0f)) return fail(SPH_ERR_ARG, "obstacle %d: size[%d] = %g must be > 0", i, a, (double)o.size[a]);
        const float* q = o.rotation;
        const float n2 = std::fma(q[3], q[3], std::fma(q[2], q[2], std::fma(q[1], q[1], q[0] * q[0])));   // (the norm obs_normalize divides by)
        if (!(n2 > 0.0f) || !std::isfinite(n2)) return fail(SPH_ERR_ARG, "obstacle %d: the quaternion is zero or cannot be normalised in fp32", i);
        if (!(o.restitution >= 0.0f && o.restitution <= 1.0f) || !(o.friction >= 0.0f && o.friction <= 1.0f))
            return fail(SPH_ERR_ARG, "obstacle %d: restitution and friction must lie in [0, 1]", i);
    }
    return SPH_OK;
}
// SphObstacle -> device record: the rotation normalised (the engine's set) or used as given (the host functions), M and the AABB built from it.
static void obstacle_to_rec(const SphObstacle& o, bool normalise, sph::ObsRec& r) {
    std::memset(&r, 0, sizeof(r));
    r.shape = o.shape;
    for (int a = 0; a < 3; ++a) { r.size[a] = o.size[a]; r.c[a] = o.center[a]; r.v[a] = o.vel[a]; r.w[a] = o.omega[a]; }
    for (int a = 0; a < 4; ++a) r.q[a] = o.rotation[a];
    r.res = o.restitution; r.fr = o.friction;
    if (normalise) sph::obs_normalize(r.q);
    sph::obs_matrix(r);
    sph::obs_extent(r);
}
static void rec_to_obstacle(const sph::ObsRec& r, SphObstacle& o) {
    o.shape = r.shape;
    for (int a = 0; a < 3; ++a) { o.size[a] = r.size[a]; o.center[a] = r.c[a]; o.vel[a] = r.v[a]; o.omega[a] = r.w[a]; }
    for (int a = 0; a < 4; ++a) o.rotation[a] = r.q[a];
    o.restitution = r.res; o.friction = r.fr;
}
static int obstacles_refuse_slab(const SphEngine* e) {
    return e->slab ? fail(SPH_ERR_STATE, "obstacles on a z-slab engine are not supported") : SPH_OK;
}
static int volumes_refuse_slab(const SphEngine* e) {
    return e->slab ? fail(SPH_ERR_STATE, "volumes on a z-slab engine are not supported") : SPH_OK;
}
static int obstacle_index_check(const SphEngine* e, int index) {
    if (index < 0 || index >= e->obsK) return fail(SPH_ERR_ARG, "obstacle index %d outside 0..%d", index, e->obsK - 1);
    return SPH_OK;
}

// The host mirror of the table to the device, stream-ordered, through the next pinned staging slot.
static int volumes_upload_table(SphEngine* e) {
    return e->d_volTab.p ? e->d_volTab.put(e, &e->volTab) : SPH_OK;
}

void sph_obstacle_default(SphObstacle* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->shape = SPH_OBSTACLE_SPHERE;
    out->size[0] = 1.0f;
    out->rotation[0] = 1.0f;
    out->restitution = 0.15f;
    out->friction = 0.02f;
}

int sph_obstacles_set(SphEngine* e, const SphObstacle* obs, int count) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = obstacles_refuse_slab(e)) || (rc = obstacles_check(obs, count))) return rc;
    if (e->volBound > 0) {                                           // (a set replaces the set: every binding goes with it)
        volumes_unbind_all(e);
        if ((rc = volumes_upload_table(e))) return rc;
    }
    if (count == 0) { obstacles_free(e); return SPH_OK; }
    if (!e->d_obs.p) {
        if ((rc = e->d_obs.ensure(e, (size_t)kObsMax, "obstacle staging")) || (rc = dev_alloc(&e->d_obsAcc, 1)) ||
            (rc = dev_alloc(&e->d_obsPart, (size_t)kObsGrid * kObsRow)) || (rc = e->d_dyn.ensure(e, (size_t)kObsMax, "obstacle staging"))) {
            obstacles_free(e); return rc;
        }
        HIP_TRY(hipMemsetAsync(e->d_dyn.p, 0, sizeof(sph::ObsDyn) * kObsMax, e->stream));
        e->obsK = 0;
    }
    if (e->dynCount > 0) {                                           // (a set replaces the set: every dynamics record goes with it)
        HIP_TRY(hipMemsetAsync(e->d_dyn.p, 0, sizeof(sph::ObsDyn) * kObsMax, e->stream));
        e->dynCount = 0;
        for (auto& on : e->dynOn) on = false;
    }
    sph::ObsRec* slot = nullptr;
    if ((rc = e->d_obs.slot(&slot))) return rc;
    for (int i = 0; i < count; ++i) obstacle_to_rec(obs[i], true, slot[i]);
    if ((rc = e->d_obs.send(e, (size_t)count))) return rc;
    if (count != e->obsK) HIP_TRY(hipMemsetAsync(e->d_obsAcc, 0, sizeof(sph::ObsAcc), e->stream));   // (another count: the sums restart)
    e->obsK = count;
    for (int i = 0; i < count; ++i) e->obsShape[i] = obs[i].shape;
    return SPH_OK;
}

int sph_obstacles_set_motion(SphEngine* e, int index, const float vel[3], const float omega[3]) {
    if (!e || !vel || !omega) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = obstacles_refuse_slab(e)) || (rc = obstacle_index_check(e, index))) return rc;
    if (!obs_all_finite(vel, 3) || !obs_all_finite(omega, 3)) return fail(SPH_ERR_ARG, "obstacle %d: velocity not finite", index);
    sph::ObsRec* slot = nullptr;
    if ((rc = e->d_obs.slot(&slot))) return rc;
    for (int a = 0; a < 3; ++a) { slot[0].v[a] = vel[a]; slot[0].w[a] = omega[a]; }
    static_assert(offsetof(sph::ObsRec, w) == offsetof(sph::ObsRec, v) + 3 * sizeof(float), "v and w are adjacent");
    return e->d_obs.send_part(e, offsetof(sph::ObsRec, v), 6 * sizeof(float), (size_t)index);   // (the pose stays the device's)
}

int sph_obstacles_get(SphEngine* e, SphObstacle* out, int cap, int* countOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (cap < e->obsK) return fail(SPH_ERR_CAPACITY, "%d obstacles (capacity %d)", e->obsK, cap);
    if (e->obsK && !out) return fail(SPH_ERR_ARG, "null argument");
    if (e->obsK) {
        sph::ObsRec host[kObsMax];
        HIP_TRY(hipMemcpyAsync(host, e->d_obs.p, sizeof(sph::ObsRec) * (size_t)e->obsK, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int i = 0; i < e->obsK; ++i) rec_to_obstacle(host[i], out[i]);
    }
    if (countOut) *countOut = e->obsK;
    return SPH_OK;
}

int sph_obstacles_impulses(SphEngine* e, double* out6, int cap, double* timeOut, uint64_t* substepsOut, int reset) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (cap < e->obsK) return fail(SPH_ERR_CAPACITY, "%d obstacles (capacity %d)", e->obsK, cap);
    sph::ObsAcc a;
    std::memset(&a, 0, sizeof(a));
    if (e->d_obsAcc) {
        HIP_TRY(hipMemcpyAsync(&a, e->d_obsAcc, sizeof(a), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (reset) HIP_TRY(hipMemsetAsync(e->d_obsAcc, 0, sizeof(sph::ObsAcc), e->stream));
    }
    if (out6 && e->obsK) std::memcpy(out6, a.J, sizeof(double) * kObsTerms * (size_t)e->obsK);
    if (timeOut) *timeOut = a.time;
    if (substepsOut) *substepsOut = a.substeps;
    return SPH_OK;
}

// The obstacle step on host records (arguments already checked): every live particle against bodies 0..count-1 in order, body b as the
// lattice vols[bindings[b]] where it is bound (bindings null: no body is; obs_hit is obs_hit_t with no lattice).
static void obstacles_apply_loop(const SphObstacle* obs, int count, const sph::VolRec* vols, const int* bindings, float particleMass,
                                 SphParticle* particles, size_t n, double* impulses6) {
    sph::ObsRec recs[kObsMax];
    for (int i = 0; i < count; ++i) obstacle_to_rec(obs[i], false, recs[i]);
    double acc[kObsRow] = {0.0};
    for (size_t i = 0; i < n; ++i) {
        SphParticle& p = particles[i];
        if (p.isGhost != 0) continue;
        float px = p.pos[0], py = p.pos[1], pz = p.pos[2], vx = p.vel[0], vy = p.vel[1], vz = p.vel[2];
        if (!std::isfinite(px) || !std::isfinite(py) || !std::isfinite(pz)) continue;
        bool changed = false;
        for (int b = 0; b < count; ++b) {
            double t[kObsTerms];
            const sph::VolRec* vol = (bindings && bindings[b] >= 0) ? &vols[bindings[b]] : nullptr;
            if (!sph::obs_hit_t<true>(recs[b], vol, particleMass, px, py, pz, vx, vy, vz, t)) continue;
            changed = true;
            for (int c = 0; c < kObsTerms; ++c) acc[b * kObsTerms + c] += t[c];
        }
        if (changed) { p.pos[0] = px; p.pos[1] = py; p.pos[2] = pz; p.vel[0] = vx; p.vel[1] = vy; p.vel[2] = vz; }
    }
    if (impulses6) std::memcpy(impulses6, acc, sizeof(double) * kObsTerms * (size_t)count);
}

int sph_obstacles_apply_host(const SphObstacle* obs, int count, float particleMass, SphParticle* particles, size_t n, double* impulses6) {
    int rc;
    if ((rc = obstacles_check(obs, count))) return rc;
    if (n && !particles) return fail(SPH_ERR_ARG, "null particles");
    obstacles_apply_loop(obs, count, nullptr, nullptr, particleMass, particles, n, impulses6);
    return SPH_OK;
}

int sph_obstacles_advance_host(SphObstacle* obs, int count, float dt) {
    int rc;
    if ((rc = obstacles_check(obs, count))) return rc;
    if (!std::isfinite(dt)) return fail(SPH_ERR_ARG, "dt not finite");
    for (int i = 0; i < count; ++i) {
        sph::ObsRec r;
        obstacle_to_rec(obs[i], false, r);
        sph::obs_advance(r, dt);
        rec_to_obstacle(r, obs[i]);
    }
    return SPH_OK;
}

// ---- active scalars: buoyancy and continuous sources (sph_couple.h) ---------
static int couple_precheck(SphEngine* e) {
    int rc;
    if ((rc = scalars_refused(e))) return rc;
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    return SPH_OK;
}
// The buffers, at the first call that switches something on.
static int couple_ensure(SphEngine* e) {
    if (e->d_cpTab.p) return SPH_OK;
    int rc;
    if ((rc = e->d_cpTab.ensure(e, 1, "pinned staging of the coupling table")) || (rc = dev_alloc(&e->d_cpAcc, 1)) ||
        (rc = dev_alloc(&e->d_cpPart, (size_t)kObsGrid * kCoupleTerms))) {
        couple_free(e);
        return rc;
    }
    HIP_TRY(hipMemsetAsync(e->d_cpAcc, 0, sizeof(sph::CoupleAcc), e->stream));
    return SPH_OK;
}
// The host mirror to the device, stream-ordered.
static int couple_upload(SphEngine* e) {
    return e->d_cpTab.p ? e->d_cpTab.put(e, &e->cpTab) : SPH_OK;
}
static int couple_clear(SphEngine* e) {
    e->cpTab = sph::CoupleTab{};
    e->cpBuoy = false;
    if (e->d_cpAcc) HIP_TRY(hipMemsetAsync(e->d_cpAcc, 0, sizeof(sph::CoupleAcc), e->stream));
    return couple_upload(e);
}
static int couple_check_sources(const SphScalarSource* src, int count, int K) {
    if (count < 0 || count > SPH_MAX_SCALAR_SOURCES) return fail(SPH_ERR_ARG, "source count %d outside 0..%d", count, SPH_MAX_SCALAR_SOURCES);
    if (count && !src) return fail(SPH_ERR_ARG, "null argument");
    for (int i = 0; i < count; ++i) {
        const SphScalarSource& s = src[i];
        if (s.shape != SPH_SOURCE_SPHERE && s.shape != SPH_SOURCE_BOX) return fail(SPH_ERR_ARG, "source %d: unknown shape %d", i, s.shape);
        if (s.mode != SPH_SOURCE_RATE && s.mode != SPH_SOURCE_RELAX) return fail(SPH_ERR_ARG, "source %d: unknown mode %d", i, s.mode);
        if (s.channel < 0 || s.channel >= K) return fail(SPH_ERR_ARG, "source %d: channel %d of %d", i, s.channel, K);
        if (s.body < -1 || s.body >= SPH_MAX_OBSTACLES) return fail(SPH_ERR_ARG, "source %d: body %d outside -1..%d", i, s.body, SPH_MAX_OBSTACLES - 1);
        if (!obs_all_finite(s.center, 3) || !obs_all_finite(s.size, 3) || !std::isfinite(s.rate) || !std::isfinite(s.target))
            return fail(SPH_ERR_ARG, "source %d: a field is not finite", i);
        const int used = s.shape == SPH_SOURCE_SPHERE ? 1 : 3;
        for (int a = 0; a < used; ++a) if (!(s.size[a] > 0.0f)) return fail(SPH_ERR_ARG, "source %d: size[%d] = %g must be > 0", i, a, (double)s.size[a]);
        if (s.rate < 0.0f) return fail(SPH_ERR_ARG, "source %d: rate %g must be >= 0", i, (double)s.rate);
    }
    return SPH_OK;
}
static int couple_check_buoyancy(const float* beta, const float* ref, int K) {
    if ((beta == nullptr) != (ref == nullptr)) return fail(SPH_ERR_ARG, "null argument");
    if (beta && (!obs_all_finite(beta, K) || !obs_all_finite(ref, K))) return fail(SPH_ERR_ARG, "a buoyancy coefficient or reference value is not finite");
    return SPH_OK;
}
static void source_to_rec(const SphScalarSource& s, sph::CoupleSrc& r) {
    std::memset(&r, 0, sizeof(r));
    r.shape = s.shape; r.channel = s.channel; r.mode = s.mode; r.body = s.body;
    for (int a = 0; a < 3; ++a) { r.center[a] = s.center[a]; r.size[a] = s.size[a]; }
    r.rate = s.rate; r.target = s.target;
}

int sph_scalars_set_buoyancy(SphEngine* e, const float* beta, const float* ref) {
    int rc;
    if ((rc = couple_precheck(e)) || (rc = couple_check_buoyancy(beta, ref, e->scK))) return rc;
    bool on = false;
    for (int k = 0; beta && k < e->scK; ++k) on = on || beta[k] != 0.0f;
    if (on && (rc = couple_ensure(e))) return rc;
    for (int k = 0; k < sph::kScalarMax; ++k) {
        e->cpTab.beta[k] = (beta && k < e->scK) ? beta[k] : 0.0f;
        e->cpTab.ref[k] = (ref && k < e->scK) ? ref[k] : 0.0f;
    }
    e->cpBuoy = on;
    return couple_upload(e);
}

int sph_scalars_get_buoyancy(SphEngine* e, float* beta, float* ref) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    for (int k = 0; k < e->scK; ++k) {
        if (beta) beta[k] = e->cpTab.beta[k];
        if (ref) ref[k] = e->cpTab.ref[k];
    }
    return SPH_OK;
}

void sph_scalar_source_default(SphScalarSource* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->shape = SPH_SOURCE_SPHERE;
    out->mode = SPH_SOURCE_RATE;
    out->body = -1;
    out->size[0] = out->size[1] = out->size[2] = 1.0f;
}

int sph_scalars_set_sources(SphEngine* e, const SphScalarSource* sources, int count) {
    int rc;
    if ((rc = couple_precheck(e)) || (rc = couple_check_sources(sources, count, e->scK))) return rc;
    if (count && (rc = couple_ensure(e))) return rc;
    if (count != e->cpTab.nSrc && e->d_cpAcc) HIP_TRY(hipMemsetAsync(e->d_cpAcc, 0, sizeof(sph::CoupleAcc), e->stream));   // (another count: the books restart)
    for (int i = 0; i < sph::kCoupleMax; ++i) {
        if (i < count) source_to_rec(sources[i], e->cpTab.src[i]);
        else std::memset(&e->cpTab.src[i], 0, sizeof(sph::CoupleSrc));
    }
    e->cpTab.nSrc = count;
    return couple_upload(e);
}

int sph_scalars_get_sources(SphEngine* e, SphScalarSource* out, int cap, int* countOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    const int count = e->cpTab.nSrc;
    if (cap < count) return fail(SPH_ERR_CAPACITY, "%d sources (capacity %d)", count, cap);
    if (count && !out) return fail(SPH_ERR_ARG, "null argument");
    if (count) std::memcpy(out, e->cpTab.src, sizeof(SphScalarSource) * (size_t)count);
    if (countOut) *countOut = count;
    return SPH_OK;
}

int sph_scalars_injected(SphEngine* e, double* sums, uint64_t* hits, int cap, double* timeOut, uint64_t* substepsOut, int reset) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (!e->scK) return fail(SPH_ERR_STATE, "no scalars: call sph_scalars_set first");
    const int count = e->cpTab.nSrc;
    if (cap < count) return fail(SPH_ERR_CAPACITY, "%d sources (capacity %d)", count, cap);
    sph::CoupleAcc a;
    std::memset(&a, 0, sizeof(a));
    if (e->d_cpAcc) {
        HIP_TRY(hipMemcpyAsync(&a, e->d_cpAcc, sizeof(a), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (reset) HIP_TRY(hipMemsetAsync(e->d_cpAcc, 0, sizeof(sph::CoupleAcc), e->stream));
    }
    for (int i = 0; i < count; ++i) {
        if (sums) sums[i] = a.sum[i];
        if (hits) hits[i] = a.hits[i];
    }
    if (timeOut) *timeOut = a.time;
    if (substepsOut) *substepsOut = a.substeps;
    return SPH_OK;
}

int sph_scalars_couple_host(SphParticle* particles, size_t n, const SphParams* params, float dt, float* values, int channels, const float* beta,
                            const float* ref, const SphScalarSource* sources, int nSources, const SphObstacle* obstacles, int nObstacles,
                            double* sumsOut, uint64_t* hitsOut) {
    if (!params || (n && (!particles || !values))) return fail(SPH_ERR_ARG, "null argument");
    if (channels < 1 || channels > SPH_MAX_SCALAR_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (1 .. %d)", channels, SPH_MAX_SCALAR_CHANNELS);
    int rc;
    if ((rc = couple_check_buoyancy(beta, ref, channels)) || (rc = couple_check_sources(sources, nSources, channels)) || (rc = obstacles_check(obstacles, nObstacles)))
        return rc;
    sph::CoupleTab tab{};
    for (int k = 0; k < channels && beta; ++k) { tab.beta[k] = beta[k]; tab.ref[k] = ref[k]; }
    tab.nSrc = nSources;
    for (int i = 0; i < nSources; ++i) {
        source_to_rec(sources[i], tab.src[i]);
        if (sources[i].body >= nObstacles) return fail(SPH_ERR_STATE, "scalar source %d rides on obstacle %d, the set has %d", i, sources[i].body, nObstacles);
    }
    sph::ObsRec recs[kObsMax];
    for (int i = 0; i < nObstacles; ++i) obstacle_to_rec(obstacles[i], false, recs[i]);
    const float step = dt > 0.0f ? dt : params->param_timeStep;
    double sums[sph::kCoupleMax] = {0.0};
    uint64_t hits[sph::kCoupleMax] = {0};
    if (!params->param_pause) {
        const float gx = params->param_gravityX, gy = params->param_gravityY, gz = params->param_gravityZ;
        const bool buoy = beta != nullptr;
        switch (channels) {
        case 1: couple_host_loop<1>(tab, buoy, recs, step, gx, gy, gz, particles, n, values, sums, hits); break;
        case 2: couple_host_loop<2>(tab, buoy, recs, step, gx, gy, gz, particles, n, values, sums, hits); break;
        case 3: couple_host_loop<3>(tab, buoy, recs, step, gx, gy, gz, particles, n, values, sums, hits); break;
        default: couple_host_loop<4>(tab, buoy, recs, step, gx, gy, gz, particles, n, values, sums, hits); break;
        }
    }
    for (int i = 0; i < nSources; ++i) {
        if (sumsOut) sumsOut[i] = sums[i];
        if (hitsOut) hitsOut[i] = hits[i];
    }
    return SPH_OK;
}

// ---- flow gates (sph_gate.h) ------------------------------------------------
static int gates_check(const SphGate* gates, int count) {
    if (count < 0 || count > SPH_MAX_GATES) return fail(SPH_ERR_ARG, "gate count %d outside 0..%d", count, SPH_MAX_GATES);
    if (count && !gates) return fail(SPH_ERR_ARG, "null argument");
    for (int i = 0; i < count; ++i) {
        const SphGate& g = gates[i];
        if (g.shape != SPH_GATE_RECT && g.shape != SPH_GATE_ELLIPSE) return fail(SPH_ERR_ARG, "gate %d: unknown shape %d", i, g.shape);
        if (g.flags & ~SPH_GATE_UNBOUNDED) return fail(SPH_ERR_ARG, "gate %d: unknown flag bits %d", i, g.flags);
        if (!obs_all_finite(g.center, 3) || !obs_all_finite(g.u, 3) || !obs_all_finite(g.v, 3)) return fail(SPH_ERR_ARG, "gate %d: a field is not finite", i);
        double uu = 0.0, vv = 0.0, uv = 0.0;
        for (int a = 0; a < 3; ++a) { uu += (double)g.u[a] * g.u[a]; vv += (double)g.v[a] * g.v[a]; uv += (double)g.u[a] * g.v[a]; }
        if (!(uu > 0.0) || !(vv > 0.0)) return fail(SPH_ERR_ARG, "gate %d: u and v must not have zero length", i);
        if (std::fabs(uv) > 1e-4 * std::sqrt(uu) * std::sqrt(vv)) return fail(SPH_ERR_ARG, "gate %d: u and v are not orthogonal (u.v = %g)", i, uv);
    }
    return SPH_OK;
}
static void gate_to_rec(const SphGate& g, sph::GateRec& r) {
    std::memset(&r, 0, sizeof(r));
    r.shape = g.shape; r.flags = g.flags;
    for (int a = 0; a < 3; ++a) { r.c[a] = g.center[a]; r.u[a] = g.u[a]; r.v[a] = g.v[a]; }
    sph::gate_derive(r);
}
// The buffers, at the first call that sets a gate; the ring grows with the history asked for.
static int gates_ensure(SphEngine* e, uint32_t history) {
    int rc;
    if (!e->d_gtTab.p) {
        if ((rc = e->d_gtTab.ensure(e, 1, "pinned staging of the gate table")) || (rc = dev_alloc(&e->d_gtAcc, 1)) ||
            (rc = e->d_gtPart.grow(e, (size_t)kGateGrid * kGateTerms))) {
            gates_free(e);
            return rc;
        }
        HIP_TRY(hipMemsetAsync(e->d_gtAcc, 0, sizeof(sph::GateAcc), e->stream));
    }
    if (history > e->gtRingCap || !e->d_gtRing.p) {
        if ((rc = e->d_gtRing.grow(e, (size_t)std::max(history, 1u) * kGateRingRow))) return rc;
        e->gtRingCap = std::max(history, 1u);
    }
    return SPH_OK;
}

int sph_gates_set(SphEngine* e, const SphGate* gates, int count, uint32_t history, uint32_t stride) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "gates on a z-slab engine are not supported: a crossing needs the entry and the exit state at one slot");
    int rc;
    if ((rc = needs_sorted_copy(e, "gates need")) || (rc = gates_check(gates, count))) return rc;
    if (history > SPH_MAX_GATE_HISTORY) return fail(SPH_ERR_ARG, "history %u above %d", history, SPH_MAX_GATE_HISTORY);
    if (stride == 0) return fail(SPH_ERR_ARG, "stride must be >= 1");
    if (!count && !e->d_gtTab.p) return SPH_OK;                        // (never set: nothing to clear)
    if ((rc = gates_ensure(e, history))) return rc;
    if (count != e->gtTab.count || history != e->gtTab.history || stride != e->gtTab.stride) {   // (another count, history or stride: books and ring restart)
        HIP_TRY(hipMemsetAsync(e->d_gtAcc, 0, sizeof(sph::GateAcc), e->stream));
        HIP_TRY(hipMemsetAsync(e->d_gtRing.p, 0, sizeof(unsigned long long) * (size_t)e->gtRingCap * kGateRingRow, e->stream));
    }
    for (int i = 0; i < sph::kGateMax; ++i) {
        if (i < count) { gate_to_rec(gates[i], e->gtTab.g[i]); e->gtSet[i] = gates[i]; }
        else { std::memset(&e->gtTab.g[i], 0, sizeof(sph::GateRec)); std::memset(&e->gtSet[i], 0, sizeof(SphGate)); }
    }
    e->gtTab.count = count; e->gtTab.history = history; e->gtTab.stride = stride;
    return e->d_gtTab.put(e, &e->gtTab);
}

int sph_gates_get(SphEngine* e, SphGate* out, int cap, int* countOut, uint32_t* historyOut, uint32_t* strideOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    const int count = e->gtTab.count;
    if (out && cap < count) return fail(SPH_ERR_CAPACITY, "%d gates (capacity %d)", count, cap);
    if (out && count) std::memcpy(out, e->gtSet, sizeof(SphGate) * (size_t)count);
    if (countOut) *countOut = count;
    if (historyOut) *historyOut = e->gtTab.history;
    if (strideOut) *strideOut = count ? e->gtTab.stride : 1u;
    return SPH_OK;
}

int sph_gates_books(SphEngine* e, SphGateBooks* books, double* timeOut, uint64_t* substepsOut, int reset) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    std::unique_ptr<sph::GateAcc> a(new sph::GateAcc());
    std::memset(a.get(), 0, sizeof(sph::GateAcc));
    if (e->d_gtAcc) {
        HIP_TRY(hipMemcpyAsync(a.get(), e->d_gtAcc, sizeof(sph::GateAcc), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (reset) HIP_TRY(hipMemsetAsync(e->d_gtAcc, 0, offsetof(sph::GateAcc, ringSteps), e->stream));   // (the ring keeps counting)
    }
    if (books && e->gtTab.count) std::memcpy(books, a->words, sizeof(SphGateBooks) * (size_t)e->gtTab.count);
    if (timeOut) *timeOut = a->time;
    if (substepsOut) *substepsOut = a->substeps;
    return SPH_OK;
}

int sph_gates_history(SphEngine* e, uint64_t* firstOut, uint32_t* countOut, SphGateBooks* rows, double* times) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    const uint32_t H = e->gtTab.count ? e->gtTab.history : 0u, S = std::max(e->gtTab.stride, 1u);
    sph::RingSpan span{0, 0};
    std::vector<unsigned long long> held;                              // the rows the ring holds, oldest first
    if (H && e->d_gtAcc) {
        unsigned long long steps = 0;
        HIP_TRY(hipMemcpyAsync(&steps, &e->d_gtAcc->ringSteps, sizeof(steps), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        span = sph::ring_span(steps / S, H);                           // one row per S counted substeps
        held.resize((size_t)span.have * kGateRingRow);
        int rc;
        if ((rc = ring_read(e, e->d_gtRing.p, sizeof(unsigned long long) * kGateRingRow, H, span, held.data()))) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    for (uint32_t i = 0; i < span.have; ++i) {
        const unsigned long long* row = held.data() + (size_t)i * kGateRingRow;
        if (rows) std::memcpy(rows + (size_t)i * e->gtTab.count, row, sizeof(SphGateBooks) * (size_t)e->gtTab.count);
        if (times) std::memcpy(times + i, row + kGateTerms, sizeof(double));
    }
    if (firstOut) *firstOut = span.first;
    if (countOut) *countOut = span.have;
    return SPH_OK;
}

int sph_gates_step_host(const SphParticle* entry, const SphParticle* exitRecords, size_t n, const SphGate* gates, int count, const float* values,
                        int channels, SphGateBooks* books) {
    if (n && (!entry || !exitRecords)) return fail(SPH_ERR_ARG, "null argument");
    if (channels < 0 || channels > SPH_MAX_SCALAR_CHANNELS) return fail(SPH_ERR_ARG, "%d channels (0 .. %d)", channels, SPH_MAX_SCALAR_CHANNELS);
    if ((channels && n && !values) || (count && !books)) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = gates_check(gates, count))) return rc;
    sph::GateRec recs[sph::kGateMax];
    for (int g = 0; g < count; ++g) gate_to_rec(gates[g], recs[g]);
    for (size_t i = 0; i < n; ++i) {
        const SphParticle& a = entry[i];
        const SphParticle& b = exitRecords[i];
        if (b.isGhost != 0 || !obs_all_finite(b.pos, 3) || !obs_all_finite(a.pos, 3)) continue;
        for (int g = 0; g < count; ++g) {
            const sph::GateRec& G = recs[g];
            const float s0 = sph::gate_side(G, a.pos[0], a.pos[1], a.pos[2]), s1 = sph::gate_side(G, b.pos[0], b.pos[1], b.pos[2]);
            const int dir = sph::gate_crossing(s0, s1);
            if (!dir || !sph::gate_counts(G, a.pos[0], a.pos[1], a.pos[2], b.pos[0], b.pos[1], b.pos[2], s0, s1)) continue;
            const double sg = dir > 0 ? 1.0 : -1.0;
            SphGateBooks& B = books[g];
            if (dir > 0) B.forward += 1; else B.backward += 1;
            for (int c = 0; c < 3; ++c) B.vel[c] += sg * (double)b.vel[c];
            for (int k = 0; k < channels; ++k) {
                const float cv = values[i * (size_t)channels + k];
                B.scalar[k] += sph::float_finite(cv) ? sg * (double)cv : 0.0;
            }
        }
    }
    return SPH_OK;
}

// ---- field monitors (sph_monitor.h) ----------------------------------------
void sph_monitor_config_default(SphMonitorConfig* out) {
    if (!out) return;
    *out = SphMonitorConfig{};
    out->every = 1u; out->wetFraction = 0.5f; out->history = 0u; out->stride = 1u; out->ringPoints = 0u;
}
static constexpr size_t kMonitorRingBytes = (size_t)256 << 20;
// The refusals every set call opens with, in the order of the gates: the engine's state before anything else, then the arguments.
static int monitor_refused(const SphEngine* e) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "monitors on a z-slab engine are not supported: its halo records after a step are the step's entry state");
    return needs_sorted_copy(e, "monitors need");
}
static int monitor_slot_check(int slot) {
    if (slot < 0 || slot >= SPH_MAX_MONITORS) return fail(SPH_ERR_ARG, "monitor slot %d outside 0..%d", slot, SPH_MAX_MONITORS - 1);
    return SPH_OK;
}
// The config against M points: *cfg is the config in force (NULL: the defaults; ringPoints 0 with a history: min(M, 64)).
static int monitor_config_check(const SphMonitorConfig* in, size_t m, SphMonitorConfig* cfg) {
    if (in) *cfg = *in; else sph_monitor_config_default(cfg);
    cfg->pad = 0u;
    if (cfg->every == 0u || cfg->stride == 0u) return fail(SPH_ERR_ARG, "every and stride must be >= 1");
    if (cfg->history > SPH_MAX_MONITOR_HISTORY) return fail(SPH_ERR_ARG, "history %u above %d", cfg->history, SPH_MAX_MONITOR_HISTORY);
    if (cfg->ringPoints > m) return fail(SPH_ERR_ARG, "ringPoints %u above the %zu points", cfg->ringPoints, m);
    if (!std::isfinite(cfg->wetFraction)) return fail(SPH_ERR_ARG, "wetFraction is not finite");
    if (cfg->history && !cfg->ringPoints) cfg->ringPoints = (uint32_t)std::min<size_t>(m, 64);
    if (!cfg->history) cfg->ringPoints = 0u;
    if ((size_t)cfg->history * cfg->ringPoints * sizeof(SphSample) > kMonitorRingBytes)
        return fail(SPH_ERR_ARG, "a ring of %u rows of %u samples exceeds 256 MiB", cfg->history, cfg->ringPoints);
    return SPH_OK;
}
// The table a set or a reset uploads: counters at zero, the first substep acts.
static sph::MonitorTab monitor_fresh_tab(const SphMonitorConfig& cfg, const sph::LatticeK& L) {
    sph::MonitorTab t{};
    t.every = cfg.every; t.stride = cfg.stride; t.history = cfg.history; t.ringPoints = cfg.ringPoints;
    t.wetFraction = cfg.wetFraction;
    t.act = 1u;
    t.row = sph::monitor_row_of(0ull, cfg.history, cfg.stride);
    t.L = L;
    return t;
}
// Rows, ring and times to zero and the fresh table to the device, stream-ordered.
static int monitor_restart(SphEngine* e, MonitorSlot& s) {
    HIP_TRY(hipMemsetAsync(s.d_rows.p, 0, s.m * sizeof(sph::MonitorRow), e->stream));
    if (s.tab.history) {
        HIP_TRY(hipMemsetAsync(s.d_ring.p, 0, (size_t)s.tab.history * s.tab.ringPoints * 2 * sizeof(float4), e->stream));
        HIP_TRY(hipMemsetAsync(s.d_times.p, 0, (size_t)s.tab.history * sizeof(double), e->stream));
    }
    return s.d_tab.put(e, &s.tab);
}
// The buffers of a slot about to hold `m` points of `kind` under cfg (arguments already checked).  A slot that keeps kind, M and ring
// layout keeps every buffer, and the graphs captured over them.
static int monitor_ensure(SphEngine* e, int slot, int kind, size_t m, const SphMonitorConfig& cfg) {
    MonitorSlot& s = e->mon[slot];
    int rc;
    const size_t ring = std::max<size_t>((size_t)cfg.history * cfg.ringPoints * 2, 1);
    if ((rc = s.d_tab.ensure(e, 1, "pinned staging of the monitor table")) || (rc = s.d_rows.grow(e, m)) || (rc = s.d_ring.grow(e, ring)) || (rc = s.d_times.grow(e, std::max<size_t>(cfg.history, 1))) ||
        (kind == SPH_MONITOR_POINTS && ((rc = s.d_points.grow(e, m)) || (rc = s.d_perm.grow(e, m))))) {
        monitor_free(e, slot);
        return rc;
    }
    return SPH_OK;
}
// The slot's host record after a successful set, then the restart.
static int monitor_commit(SphEngine* e, int slot, int kind, size_t m, const int dims[3], const float origin[3], const float spacing[3],
                          const SphMonitorConfig& cfg, const sph::LatticeK& L) {
    MonitorSlot& s = e->mon[slot];
    if (s.kind == SPH_MONITOR_NONE) e->monCount += 1;
    s.kind = kind; s.m = m; s.cfg = cfg;
    for (int a = 0; a < 3; ++a) { s.dims[a] = dims[a]; s.origin[a] = origin[a]; s.spacing[a] = spacing[a]; }
    s.tab = monitor_fresh_tab(cfg, L);
    return monitor_restart(e, s);
}
// The processing order of explicit points: sorted by the cell of the grid in force at set time (speed only; the points never move).
static void monitor_order(const SphEngine* e, const float4* pts, size_t m, std::vector<uint32_t>& perm) {
    SphGridInfo g{};
    sph::compute_grid_extents(e->params, g);
    perm.resize(m);
    for (size_t i = 0; i < m; ++i) perm[i] = (uint32_t)i;
    if (!(g.cellSize > 0.0f) || !std::isfinite(g.cellSize)) return;
    std::vector<uint32_t> cell(m);
    for (size_t i = 0; i < m; ++i) {
        const float p[3] = {pts[i].x, pts[i].y, pts[i].z};
        int c[3];
        for (int a = 0; a < 3; ++a) {
            const float f = std::floor((p[a] - g.gridMin[a]) / g.cellSize);
            c[a] = !(f >= 0.0f) ? 0 : (f >= (float)(g.dims[a] - 1) ? std::max(g.dims[a] - 1, 0) : (int)f);
        }
        cell[i] = (uint32_t)((c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0]);
    }
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return cell[a] < cell[b]; });
}
static int monitor_set_points(SphEngine* e, int slot, const float* points4, size_t m, const SphMonitorConfig* config, bool onDevice) {
    int rc;
    SphMonitorConfig cfg;
    if ((rc = monitor_refused(e)) || (rc = monitor_slot_check(slot))) return rc;
    if (m && !points4) return fail(SPH_ERR_ARG, "null argument");
    if (m > (size_t)SPH_MAX_MONITOR_POINTS) return fail(SPH_ERR_ARG, "%zu monitor points exceed %d", m, SPH_MAX_MONITOR_POINTS);
    if ((rc = monitor_config_check(config, m ? m : 1, &cfg))) return rc;
    if (m == 0) { monitor_free(e, slot); return SPH_OK; }
    std::vector<float4> host(m);
    if (onDevice) {                                                    // (the order is made on the host: a set call is rare)
        HIP_TRY(hipMemcpyAsync(host.data(), points4, m * sizeof(float4), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    } else {
        std::memcpy(host.data(), points4, m * sizeof(float4));
    }
    std::vector<uint32_t> perm;
    monitor_order(e, host.data(), m, perm);
    if ((rc = monitor_ensure(e, slot, SPH_MONITOR_POINTS, m, cfg))) return rc;
    MonitorSlot& s = e->mon[slot];
    HIP_TRY(hipMemcpyAsync(s.d_points.p, host.data(), m * sizeof(float4), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(s.d_perm.p, perm.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    const int dims[3] = {(int)m, 1, 1};
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    rc = monitor_commit(e, slot, SPH_MONITOR_POINTS, m, dims, zero, zero, cfg, sph::LatticeK{});
    HIP_TRY(hipStreamSynchronize(e->stream));                          // (the two vectors are pageable memory)
    return rc;
}
int sph_monitor_set(SphEngine* e, int slot, const float* points4, size_t m, const SphMonitorConfig* config) {
    return monitor_set_points(e, slot, points4, m, config, false);
}
int sph_monitor_set_device(SphEngine* e, int slot, const float* devPoints4, size_t m, const SphMonitorConfig* config) {
    return monitor_set_points(e, slot, devPoints4, m, config, true);
}
int sph_monitor_set_lattice(SphEngine* e, int slot, const float origin[3], const float spacing[3], const int dims[3], const SphMonitorConfig* config) {
    int rc;
    SphMonitorConfig cfg;
    long long total = 0;
    if ((rc = monitor_refused(e)) || (rc = monitor_slot_check(slot))) return rc;
    if (!origin || !spacing || !dims) return fail(SPH_ERR_ARG, "null argument");
    if ((rc = check_lattice(dims, spacing, 1, &total))) return rc;
    if (total > (long long)SPH_MAX_MONITOR_POINTS) return fail(SPH_ERR_ARG, "a lattice of %lld monitor points exceeds %d", total, SPH_MAX_MONITOR_POINTS);
    if (!obs_all_finite(origin, 3)) return fail(SPH_ERR_ARG, "the lattice origin is not finite");
    if ((rc = monitor_config_check(config, (size_t)total, &cfg))) return rc;
    if ((rc = monitor_ensure(e, slot, SPH_MONITOR_LATTICE, (size_t)total, cfg))) return rc;
    return monitor_commit(e, slot, SPH_MONITOR_LATTICE, (size_t)total, dims, origin, spacing, cfg, lattice_consts(origin, spacing, dims, SPH_FIELD_ALL, kSampleStage));
}
// The device's counters of a slot that holds a monitor.  Synchronises.
static int monitor_counters(SphEngine* e, const MonitorSlot& s, sph::MonitorTab* out) {
    HIP_TRY(hipMemcpyAsync(out, s.d_tab.p, sizeof(sph::MonitorTab), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}
// The ring rows a slot still holds: one per `stride` acting substeps, the first acting substep writing row 0.
static sph::RingSpan monitor_ring_span(const sph::MonitorTab& t) {
    return sph::ring_span(t.history ? (t.a + t.stride - 1) / t.stride : 0, t.history);
}
int sph_monitor_info(SphEngine* e, int slot, SphMonitorInfo* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    std::memset(out, 0, sizeof(*out));
    const MonitorSlot& s = e->mon[slot];
    if (s.kind == SPH_MONITOR_NONE) return SPH_OK;
    sph::MonitorTab t;
    if ((rc = monitor_counters(e, s, &t))) return rc;
    out->kind = s.kind; out->points = s.m; out->config = s.cfg;
    for (int a = 0; a < 3; ++a) { out->dims[a] = s.dims[a]; out->origin[a] = s.origin[a]; out->spacing[a] = s.spacing[a]; }
    out->substeps = t.c; out->acting = t.a; out->time = t.time;
    const sph::RingSpan span = monitor_ring_span(t);
    out->firstRow = span.first; out->ringRows = span.have;
    return SPH_OK;
}
int sph_monitor_download(SphEngine* e, int slot, SphMonitorRow* out, size_t cap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    const MonitorSlot& s = e->mon[slot];
    if (cap < s.m) return fail(SPH_ERR_CAPACITY, "%zu monitor rows (capacity %zu)", s.m, cap);
    if (s.m && !out) return fail(SPH_ERR_ARG, "null argument");
    if (s.m) HIP_TRY(hipMemcpyAsync(out, s.d_rows.p, s.m * sizeof(SphMonitorRow), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}
int sph_monitor_device(SphEngine* e, int slot, const SphMonitorRow** devPtr) {
    if (!e || !devPtr) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    *devPtr = e->mon[slot].kind != SPH_MONITOR_NONE ? reinterpret_cast<const SphMonitorRow*>(e->mon[slot].d_rows.p) : nullptr;
    return SPH_OK;
}
int sph_monitor_history(SphEngine* e, int slot, uint64_t* firstOut, uint32_t* countOut, SphSample* samples, double* times, size_t rowCap) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    const MonitorSlot& s = e->mon[slot];
    sph::RingSpan span{0, 0};
    if (s.kind != SPH_MONITOR_NONE && s.tab.history) {
        sph::MonitorTab t;
        if ((rc = monitor_counters(e, s, &t))) return rc;
        span = monitor_ring_span(t);
        if ((samples || times) && rowCap < span.have) return fail(SPH_ERR_CAPACITY, "%u ring rows (capacity %zu)", span.have, rowCap);
        if (samples && (rc = ring_read(e, s.d_ring.p, (size_t)t.ringPoints * sizeof(SphSample), t.history, span, samples))) return rc;
        if (times && (rc = ring_read(e, s.d_times.p, sizeof(double), t.history, span, times))) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (firstOut) *firstOut = span.first;
    if (countOut) *countOut = span.have;
    return SPH_OK;
}
int sph_monitor_field(SphEngine* e, int slot, int field, float* devOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    if (field < 0 || field >= sph::kMonFields) return fail(SPH_ERR_ARG, "unknown monitor field %d", field);
    const MonitorSlot& s = e->mon[slot];
    if (s.kind == SPH_MONITOR_NONE) return fail(SPH_ERR_STATE, "no monitor in slot %d", slot);
    if (!devOut) return fail(SPH_ERR_ARG, "null argument");
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_monitor_field, dim3(blocks_for(s.m)), dim3(kBlock), 0, e->stream, (const sph::MonitorRow*)s.d_rows.p, field, devOut, s.m);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}
int sph_monitor_reset(SphEngine* e, int slot) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = monitor_slot_check(slot))) return rc;
    MonitorSlot& s = e->mon[slot];
    if (s.kind == SPH_MONITOR_NONE) return fail(SPH_ERR_STATE, "no monitor in slot %d", slot);
    return monitor_restart(e, s);                                      // (s.tab is the table of the last set: counters at zero)
}
int sph_monitor_clear(SphEngine* e, int slot) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (slot >= SPH_MAX_MONITORS) return monitor_slot_check(slot);
    if (slot < 0) monitors_free(e); else monitor_free(e, slot);
    return SPH_OK;
}
int sph_monitor_accumulate_host(SphMonitorRow* rows, const SphSample* samples, size_t m, float wetFraction) {
    if (m && (!rows || !samples)) return fail(SPH_ERR_ARG, "null argument");
    if (!std::isfinite(wetFraction)) return fail(SPH_ERR_ARG, "wetFraction is not finite");
    for (size_t i = 0; i < m; ++i) {
        const SphSample& q = samples[i];
        (void)sph::monitor_update(*reinterpret_cast<sph::MonitorRow*>(rows + i), q.density, q.fraction, q.pressure, q.vel[0], q.vel[1], q.vel[2], wetFraction);
    }
    return SPH_OK;
}
int sph_monitor_field_host(const SphMonitorRow* rows, size_t m, int field, float* out) {
    if (m && (!rows || !out)) return fail(SPH_ERR_ARG, "null argument");
    if (field < 0 || field >= sph::kMonFields) return fail(SPH_ERR_ARG, "unknown monitor field %d", field);
    for (size_t i = 0; i < m; ++i) out[i] = sph::monitor_field_value(*reinterpret_cast<const sph::MonitorRow*>(rows + i), field);
    return SPH_OK;
}
int sph_monitor_schedule_host(uint32_t every, uint32_t stride, uint32_t history, size_t substeps, uint32_t* actsOut, uint32_t* rowsOut) {
    if (substeps && (!actsOut || !rowsOut)) return fail(SPH_ERR_ARG, "null argument");
    if (every == 0u || stride == 0u) return fail(SPH_ERR_ARG, "every and stride must be >= 1");
    if (history > SPH_MAX_MONITOR_HISTORY) return fail(SPH_ERR_ARG, "history %u above %d", history, SPH_MAX_MONITOR_HISTORY);
    SphMonitorConfig cfg{};
    cfg.every = every; cfg.stride = stride; cfg.history = history; cfg.ringPoints = history ? 1u : 0u;
    sph::MonitorTab t = monitor_fresh_tab(cfg, sph::LatticeK{});
    for (size_t i = 0; i < substeps; ++i) {
        bool acted;
        rowsOut[i] = sph::monitor_tick(t, 0.0, &acted);
        actsOut[i] = acted ? 1u : 0u;
    }
    return SPH_OK;
}

// ---- dynamic bodies (sph_obstacle.h obs_body_step) --------------------------
void sph_obstacle_dynamics_default(SphObstacleDynamics* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->mass = 1.0f;
    out->inertia[0] = out->inertia[1] = out->inertia[2] = 1.0f;
    out->gravityScale = 1.0f;
    out->flags = SPH_DYNAMICS_CONFINED;
}
// Checks a record and builds the device record: the inertia inverted in fp64 (adjugate over determinant), both stored as fp32.
static int dynamics_to_rec(const SphObstacleDynamics& d, int index, sph::ObsDyn& r) {
    const float* f = &d.mass;
    static_assert(offsetof(SphObstacleDynamics, flags) == 19 * sizeof(float), "nineteen floats, then the flags");
    if (!obs_all_finite(f, 19)) return fail(SPH_ERR_ARG, "obstacle %d: a dynamics field is not finite", index);
    if (!(d.mass > 0.0f)) return fail(SPH_ERR_ARG, "obstacle %d: mass %g must be > 0", index, (double)d.mass);
    if (d.linearDamping < 0.0f || d.angularDamping < 0.0f) return fail(SPH_ERR_ARG, "obstacle %d: a damping is negative", index);
    const double xx = d.inertia[0], yy = d.inertia[1], zz = d.inertia[2], xy = d.inertia[3], xz = d.inertia[4], yz = d.inertia[5];
    const double m2 = xx * yy - xy * xy;
    const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
    const double det = xx * c00 + xy * c01 + xz * c02;
    if (!(xx > 0.0) || !(m2 > 0.0) || !(det > 0.0) || !std::isfinite(det))                      // (Sylvester's criterion)
        return fail(SPH_ERR_ARG, "obstacle %d: the inertia tensor is not positive definite", index);
    const double inv[6] = {c00 / det, (xx * zz - xz * xz) / det, m2 / det, c01 / det, c02 / det, (xy * xz - xx * yz) / det};
    std::memset(&r, 0, sizeof(r));
    r.active = 1;
    r.mass = d.mass;
    for (int a = 0; a < 6; ++a) { r.I[a] = d.inertia[a]; r.Iinv[a] = (float)inv[a]; }
    if (!obs_all_finite(r.Iinv, 6)) return fail(SPH_ERR_ARG, "obstacle %d: the inverse inertia is not finite in fp32", index);
    for (int a = 0; a < 3; ++a) { r.com[a] = d.com[a]; r.force[a] = d.force[a]; r.torque[a] = d.torque[a]; }
    r.gscale = d.gravityScale;
    r.ldamp = d.linearDamping; r.adamp = d.angularDamping;
    r.flags = d.flags;
    return SPH_OK;
}

int sph_obstacles_set_dynamics(SphEngine* e, int index, const SphObstacleDynamics* dyn) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = obstacles_refuse_slab(e)) || (rc = obstacle_index_check(e, index))) return rc;
    sph::ObsDyn rec;
    std::memset(&rec, 0, sizeof(rec));
    if (dyn && (rc = dynamics_to_rec(*dyn, index, rec))) return rc;
    if ((rc = e->d_dyn.put(e, &rec, 1, (size_t)index))) return rc;
    const bool on = dyn != nullptr;
    e->dynCount += (on ? 1 : 0) - (e->dynOn[index] ? 1 : 0);
    e->dynOn[index] = on;
    if (on) e->dynSet[index] = *dyn;
    return SPH_OK;
}

int sph_obstacles_get_dynamics(SphEngine* e, int index, SphObstacleDynamics* out, int* dynamicOut) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = obstacle_index_check(e, index))) return rc;
    if (out) {
        if (e->dynOn[index]) *out = e->dynSet[index];
        else sph_obstacle_dynamics_default(out);
    }
    if (dynamicOut) *dynamicOut = e->dynOn[index] ? 1 : 0;
    return SPH_OK;
}

int sph_obstacles_step_host(SphObstacle* obs, const SphObstacleDynamics* dyn, int count, const double* impulses6, const SphParams* params, float dt) {
    int rc;
    if ((rc = obstacles_check(obs, count))) return rc;
    if (!params || (count && !dyn)) return fail(SPH_ERR_ARG, "null argument");
    if (!std::isfinite(dt)) return fail(SPH_ERR_ARG, "dt not finite");
    sph::ObsDyn recs[kObsMax];
    for (int i = 0; i < count; ++i) {
        std::memset(&recs[i], 0, sizeof(recs[i]));
        if (dyn[i].mass != 0.0f && (rc = dynamics_to_rec(dyn[i], i, recs[i]))) return rc;
    }
    sph::ObsWorld W;
    obstacle_world(*params, W);
    const double zero[kObsTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < count; ++i) {
        sph::ObsRec r;
        obstacle_to_rec(obs[i], false, r);
        if (recs[i].active) sph::obs_body_step(r, recs[i], impulses6 ? impulses6 + (size_t)i * kObsTerms : zero, W, dt);
        else sph::obs_advance(r, dt);
        rec_to_obstacle(r, obs[i]);
    }
    return SPH_OK;
}

// ---- volumes: signed distance lattices as bodies, mesh -> signed distance (sph_volume.h) ---------
// A free slot and, on the first call, the device table with its staging.
static int volume_free_slot(SphEngine* e, int* idOut) {
    int rc, id = -1;
    for (int i = 0; i < kVolMax; ++i) if (!e->vols[i].d) { id = i; break; }
    if (id < 0) return fail(SPH_ERR_CAPACITY, "all %d volume slots are in use", kVolMax);
    if ((rc = e->d_volTab.ensure(e, 1, "volume staging"))) return rc;
    *idOut = id;
    return SPH_OK;
}
// The engine takes the device array d as volume `id`.
static int volume_adopt(SphEngine* e, int id, float* d, const int dims[3], const float spacing[3]) {
    SphEngine::VolSlot& v = e->vols[id];
    v.d = d;
    for (int a = 0; a < 3; ++a) { v.dims[a] = dims[a]; v.spacing[a] = spacing[a]; }
    sph::vol_make(d, dims, spacing, e->volTab.vol[id]);
    return volumes_upload_table(e);
}

int sph_volume_create(SphEngine* e, const float* values, const int dims[3], const float spacing[3], int onDevice, int* idOut) {
    if (!e || !values || !idOut) return fail(SPH_ERR_ARG, "null argument");
    int rc, id = -1;
    long long total = 0;
    if ((rc = volumes_refuse_slab(e)) || (rc = check_lattice(dims, spacing, 2, &total)) || (rc = volume_free_slot(e, &id))) return rc;
    float* d = nullptr;
    if ((rc = dev_alloc(&d, (size_t)total))) return rc;
    hipError_t er = hipMemcpyAsync(d, values, (size_t)total * sizeof(float), onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream);
    if (er == hipSuccess && !onDevice) er = hipStreamSynchronize(e->stream);      // (the caller's host array is free on return)
    if (er != hipSuccess) { dev_free(d); return fail(SPH_ERR_HIP, "volume upload: %s", hipGetErrorString(er)); }
    if ((rc = volume_adopt(e, id, d, dims, spacing))) return rc;
    *idOut = id;
    return SPH_OK;
}

static int volume_slot_check(const SphEngine* e, int id) {
    if (id < 0 || id >= kVolMax || !e->vols[id].d) return fail(SPH_ERR_ARG, "volume %d does not exist", id);
    return SPH_OK;
}

int sph_volume_destroy(SphEngine* e, int id) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = volume_slot_check(e, id))) return rc;
    for (int i = 0; i < e->obsK; ++i)
        if (e->volTab.bind[i] == id) return fail(SPH_ERR_STATE, "volume %d is bound to obstacle %d", id, i);
    HIP_TRY(hipStreamSynchronize(e->stream));                        // (queued substeps or builds may still read it)
    dev_free(e->vols[id].d);
    e->vols[id] = SphEngine::VolSlot{};
    std::memset(&e->volTab.vol[id], 0, sizeof(sph::VolRec));
    return volumes_upload_table(e);
}

int sph_volume_info(SphEngine* e, int id, int dimsOut[3], float spacingOut[3], float halfOut[3]) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = volume_slot_check(e, id))) return rc;
    for (int a = 0; a < 3; ++a) {
        if (dimsOut) dimsOut[a] = e->vols[id].dims[a];
        if (spacingOut) spacingOut[a] = e->vols[id].spacing[a];
        if (halfOut) halfOut[a] = e->volTab.vol[id].half[a];
    }
    return SPH_OK;
}

int sph_volume_moments(SphEngine* e, int id, double out[10]) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = volume_slot_check(e, id))) return rc;
    if ((rc = e->d_momPart.grow(e, (size_t)kMomGrid * kMomTerms)) || (rc = e->d_momOut.grow(e, (size_t)kMomTerms))) return rc;
    const sph::VolRec& v = e->volTab.vol[id];
    const long long total = (long long)v.dims[0] * v.dims[1] * v.dims[2];
    const int rows = (int)std::min<long long>(kMomGrid, (total + kMomSweep - 1) / kMomSweep);
    const double cell = ((double)v.spacing[0] * (double)v.spacing[1]) * (double)v.spacing[2];
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_volume_moments, dim3(rows), dim3(kMomBlock), 0, e->stream, v, sph::vol_diagonal(v.spacing), (unsigned)total, e->d_momPart.p);
        hipLaunchKernelGGL(k_volume_moments_finish, dim3(1), dim3(kMomFinishBlock), 0, e->stream, (const double*)e->d_momPart.p, rows, cell, e->d_momOut.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, e->d_momOut.p, sizeof(double) * kMomTerms, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

int sph_volume_moments_host(const float* values, const int dims[3], const float spacing[3], double out[10]) {
    if (!values || !out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = check_lattice(dims, spacing, 2, nullptr))) return rc;
    sph::VolRec v;
    sph::vol_make(values, dims, spacing, v);
    const float diag = sph::vol_diagonal(v.spacing);
    double t[kMomTerms] = {0.0};
    size_t p = 0;
    for (int k = 0; k < dims[2]; ++k)
        for (int j = 0; j < dims[1]; ++j)
            for (int i = 0; i < dims[0]; ++i, ++p)
                sph::vol_moment_terms(values[p], diag, (float)i * v.spacing[0] - v.half[0], (float)j * v.spacing[1] - v.half[1],
                                      (float)k * v.spacing[2] - v.half[2], t);
    const double cell = ((double)spacing[0] * (double)spacing[1]) * (double)spacing[2];
    for (int c = 0; c < kMomTerms; ++c) out[c] = t[c] * cell;
    return SPH_OK;
}

int sph_obstacles_bind_volume(SphEngine* e, int index, int id) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = volumes_refuse_slab(e)) || (rc = obstacle_index_check(e, index))) return rc;
    if (id >= 0) {
        if ((rc = volume_slot_check(e, id))) return rc;
        if (e->obsShape[index] != SPH_OBSTACLE_BOX) return fail(SPH_ERR_ARG, "obstacle %d is not a box: a volume binds to SPH_OBSTACLE_BOX only", index);
    } else {
        id = -1;
    }
    if (e->volTab.bind[index] == id) return SPH_OK;
    e->volBound += (id >= 0 ? 1 : 0) - (e->volTab.bind[index] >= 0 ? 1 : 0);
    e->volTab.bind[index] = id;
    return volumes_upload_table(e);
}

int sph_obstacles_volume(SphEngine* e, int index, int* idOut) {
    if (!e || !idOut) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = obstacle_index_check(e, index))) return rc;
    *idOut = e->volTab.bind[index];
    return SPH_OK;
}

static int volume_host_check(const SphVolumeHost& v) {
    if (!v.values) return fail(SPH_ERR_ARG, "null lattice values");
    return check_lattice(v.dims, v.spacing, 2, nullptr);
}

int sph_volume_sample_host(const float* values, const int dims[3], const float spacing[3], const float local[3], float* phiOut, float gradOut[3],
                           int* insideOut) {
    if (!values || !local || !phiOut || !gradOut || !insideOut) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = check_lattice(dims, spacing, 2, nullptr))) return rc;
    sph::VolRec v;
    sph::vol_make(values, dims, spacing, v);
    float phi = std::nanf(""), g[3] = {0.0f, 0.0f, 0.0f};
    const bool in = sph::vol_sample(v, local[0], local[1], local[2], false, phi, g);
    if (!in) { const uint32_t q = 0x7FC00000u; std::memcpy(&phi, &q, 4); g[0] = g[1] = g[2] = 0.0f; }
    *phiOut = phi;
    for (int a = 0; a < 3; ++a) gradOut[a] = g[a];
    *insideOut = in && phi < 0.0f ? 1 : 0;
    return SPH_OK;
}

int sph_obstacles_apply_host_volumes(const SphObstacle* obs, int count, const SphVolumeHost* volumes, int volumeCount, const int* bindings,
                                     float particleMass, SphParticle* particles, size_t n, double* impulses6) {
    int rc;
    if ((rc = obstacles_check(obs, count))) return rc;
    if (volumeCount < 0 || volumeCount > SPH_MAX_VOLUMES) return fail(SPH_ERR_ARG, "volume count %d outside 0..%d", volumeCount, SPH_MAX_VOLUMES);
    if ((volumeCount && !volumes) || (count && !bindings)) return fail(SPH_ERR_ARG, "null argument");
    if (n && !particles) return fail(SPH_ERR_ARG, "null particles");
    sph::VolRec vols[kVolMax];
    for (int i = 0; i < volumeCount; ++i) {
        if ((rc = volume_host_check(volumes[i]))) return rc;
        sph::vol_make(volumes[i].values, volumes[i].dims, volumes[i].spacing, vols[i]);
    }
    for (int i = 0; i < count; ++i) {
        if (bindings[i] < 0) continue;
        if (bindings[i] >= volumeCount) return fail(SPH_ERR_ARG, "obstacle %d: volume %d outside 0..%d", i, bindings[i], volumeCount - 1);
        if (obs[i].shape != SPH_OBSTACLE_BOX) return fail(SPH_ERR_ARG, "obstacle %d is not a box: a volume binds to SPH_OBSTACLE_BOX only", i);
    }
    obstacles_apply_loop(obs, count, vols, bindings, particleMass, particles, n, impulses6);
    return SPH_OK;
}

static int mesh_check(const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float origin[3], const float spacing[3],
                      const int dims[3], long long* totalOut) {
    if (!vertices3 || !triangles3 || !origin) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    if ((rc = check_lattice(dims, spacing, 1, totalOut))) return rc;                       // (a lattice of points as in sph_sample_lattice: dims >= 1)
    if (nt == 0 || nt > 2147483647ull / 3 || nv == 0 || nv > 0xFFFFFFFFull) return fail(SPH_ERR_ARG, "a mesh of %zu vertices and %zu triangles", nv, nt);
    if (!obs_all_finite(origin, 3)) return fail(SPH_ERR_ARG, "lattice origin not finite");
    for (size_t i = 0; i < 3 * nv; ++i) if (!std::isfinite(vertices3[i])) return fail(SPH_ERR_ARG, "vertex %zu is not finite", i / 3);
    for (size_t i = 0; i < 3 * nt; ++i) if (triangles3[i] >= nv) return fail(SPH_ERR_ARG, "triangle %zu names vertex %u of %zu", i / 3, triangles3[i], nv);
    return SPH_OK;
}

int sph_mesh_distance(SphEngine* e, const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float origin[3],
                      const float spacing[3], const int dims[3], float* devOut) {
    if (!e || !devOut) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    long long total = 0;
    if ((rc = mesh_check(vertices3, nv, triangles3, nt, origin, spacing, dims, &total))) return rc;
    const long long blocks = (total + kMeshBlock - 1) / kMeshBlock;
    // the triangles are split until about 2048 blocks exist (8 per compute unit), never below one chunk per split
    int splits = e->optMeshSplit;
    if (splits <= 0) splits = (int)std::min<long long>(64, std::max<long long>(1, 2048 / blocks));
    splits = (int)std::min<size_t>((size_t)splits, (nt + kMeshChunk - 1) / kMeshChunk);
    splits = std::max(1, std::min(splits, 64));
    const int per = (int)((nt + (size_t)splits - 1) / (size_t)splits);
    const size_t part = (size_t)splits * (size_t)total;
    if ((rc = e->d_meshVerts.grow(e, 3 * nv)) || (rc = e->d_meshTris.grow(e, 3 * nt)) || (rc = e->d_meshD2.grow(e, part)) || (rc = e->d_meshW.grow(e, part))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_meshVerts.p, vertices3, 3 * nv * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_meshTris.p, triangles3, 3 * nt * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    sph::MeshLattice L;
    L.ox = origin[0]; L.oy = origin[1]; L.oz = origin[2];
    L.sx = spacing[0]; L.sy = spacing[1]; L.sz = spacing[2];
    L.nx = dims[0]; L.ny = dims[1]; L.nz = dims[2];
    L.total = total;
    {
        Timed t(e, SPH_K_OTHER);
        hipLaunchKernelGGL(k_mesh_distance, dim3((unsigned)blocks, (unsigned)splits), dim3(kMeshBlock), 0, e->stream, (const float*)e->d_meshVerts.p,
                           (const uint32_t*)e->d_meshTris.p, (int)nt, per, L, e->d_meshD2.p, e->d_meshW.p);
        hipLaunchKernelGGL(k_mesh_merge, dim3((unsigned)blocks), dim3(kMeshBlock), 0, e->stream, (const float*)e->d_meshD2.p, (const double*)e->d_meshW.p, splits,
                           total, devOut);
    }
    HIP_TRY(hipGetLastError());
    return SPH_OK;
}

int sph_volume_from_mesh(SphEngine* e, const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float center[3],
                         const float spacing[3], const int dims[3], int* idOut) {
    if (!e || !center || !idOut) return fail(SPH_ERR_ARG, "null argument");
    int rc, id = -1;
    long long total = 0;
    if ((rc = volumes_refuse_slab(e)) || (rc = check_lattice(dims, spacing, 2, &total)) || (rc = mesh_check(vertices3, nv, triangles3, nt, center, spacing, dims, &total)) ||
        (rc = volume_free_slot(e, &id))) return rc;
    float origin[3];
    for (int a = 0; a < 3; ++a) origin[a] = center[a] - (0.5f * (float)(dims[a] - 1)) * spacing[a];
    float* d = nullptr;
    if ((rc = dev_alloc(&d, (size_t)total))) return rc;
    if ((rc = sph_mesh_distance(e, vertices3, nv, triangles3, nt, origin, spacing, dims, d))) { dev_free(d); return rc; }
    if ((rc = volume_adopt(e, id, d, dims, spacing))) return rc;
    *idOut = id;
    return SPH_OK;
}

int sph_mesh_distance_host(const float* vertices3, size_t nv, const uint32_t* triangles3, size_t nt, const float origin[3], const float spacing[3],
                           const int dims[3], float* out) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    int rc;
    long long total = 0;
    if ((rc = mesh_check(vertices3, nv, triangles3, nt, origin, spacing, dims, &total))) return rc;
    std::vector<sph::MeshTri> tris(nt);
    for (size_t t = 0; t < nt; ++t) sph::mesh_tri_setup(vertices3, triangles3 + 3 * t, tris[t]);
    size_t p = 0;
    for (int k = 0; k < dims[2]; ++k)
        for (int j = 0; j < dims[1]; ++j)
            for (int i = 0; i < dims[0]; ++i, ++p) {
                const float x = origin[0] + (float)i * spacing[0], y = origin[1] + (float)j * spacing[1], z = origin[2] + (float)k * spacing[2];
                float best = INFINITY;
                double angles = 0.0;
                for (size_t t = 0; t < nt; ++t) {
                    const float d2 = sph::mesh_tri_d2(tris[t], x, y, z);
                    if (d2 < best) best = d2;
                    angles += (double)sph::mesh_tri_angle(tris[t], x, y, z);
                }
                out[p] = sph::mesh_signed(best, angles);
            }
    return SPH_OK;
}

int sph_kernel_times(SphEngine* e, double msOut[SPH_K_COUNT], int64_t launchesOut[SPH_K_COUNT], int reset) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    int rc;
    if ((rc = flush_events(e))) return rc;
    for (int i = 0; i < SPH_K_COUNT; ++i) {
        if (msOut) msOut[i] = e->kms[i];
        if (launchesOut) launchesOut[i] = e->klaunch[i];
        if (reset) { e->kms[i] = 0.0; e->klaunch[i] = 0; }
    }
    return SPH_OK;
}

// ---- checkpoints (sph_state.h) ------------------------------------------------
static_assert(offsetof(sph::MonitorTab, c) == 0 && offsetof(sph::MonitorTab, a) == 8 && offsetof(sph::MonitorTab, time) == 16, "the counters lead the monitor table");
static_assert(sizeof(sph::GateAcc) % 8 == 0 && sizeof(SphTracer) == 32 && sizeof(SphSample) == 32, "checkpoint pieces are 64-bit words");

// One section as the pieces it is made of, in order: bytes the host holds, or an array in device memory (a multiple of 8 bytes each).
// sph_state_size sums them, sph_state_save copies them, sph_state_digest hashes them where they lie.
namespace {
struct StatePiece {
    std::vector<unsigned char> host;
    const void* dev = nullptr;
    size_t bytes = 0;
};
struct StateSection {
    uint32_t tag = 0;
    std::vector<StatePiece> pieces;
    size_t bytes() const { size_t b = 0; for (const StatePiece& p : pieces) b += p.bytes; return b; }
    void add_host(const void* p, size_t n) {
        if (pieces.empty() || pieces.back().dev) pieces.emplace_back();
        const unsigned char* c = static_cast<const unsigned char*>(p);
        pieces.back().host.insert(pieces.back().host.end(), c, c + n);
        pieces.back().bytes = pieces.back().host.size();
    }
    void add_dev(const void* p, size_t n) {
        if (!n) return;
        pieces.emplace_back();
        pieces.back().dev = p; pieces.back().bytes = n;
    }
    // A device array of 32-bit words: the whole 64-bit words where they lie, an odd last word as a host piece (with four zero bytes, the
    // blob's padding), read from the device only if `read` (sizes do not need it).
    int add_dev32(SphEngine* e, const void* p, size_t words, bool read) {
        add_dev(p, (words & ~(size_t)1) * 4u);
        if (words & 1u) {
            uint32_t last[2] = {0u, 0u};
            if (read) {
                HIP_TRY(hipMemcpyAsync(last, static_cast<const uint32_t*>(p) + (words - 1), 4, hipMemcpyDeviceToHost, e->stream));
                HIP_TRY(hipStreamSynchronize(e->stream));
            }
            add_host(last, 8);
        }
        return SPH_OK;
    }
};
}  // namespace

static void state_tracer_words(uint64_t steps, uint32_t K, uint32_t S, uint32_t out[3]) {
    out[0] = (uint32_t)steps; out[1] = (uint32_t)(steps >> 32);
    out[2] = sph::tracer_slot_of(steps + 1ull, K, S);
}

// The sections of the engine as it stands.  current: also bring the 80-byte records up to date (a launch; sizes do not need it).
static int state_collect(SphEngine* e, bool current, std::vector<StateSection>& out) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "checkpoints of a z-slab engine are not supported: its state is one share of a decomposed run");
    if (e->n == 0) return fail(SPH_ERR_STATE, "an engine without particles has no checkpoint");
    int rc;
    if (current && (rc = writeback(e))) return rc;
    out.clear();
    {
        StateSection s;
        s.tag = SPH_STATE_CORE;
        sph::StateCore c;
        std::memset(&c, 0, sizeof(c));
        c.params = e->params; c.lastDt = e->lastDt; c.fountain = e->fountain; c.river = e->river;
        c.terrainCount = e->terrainHeights.size(); c.stencilCount = e->d_stencil ? e->stencilCount : 0;
        s.add_host(&c, sizeof(c));
        if (c.terrainCount) {
            s.add_host(e->terrainHeights.data(), c.terrainCount * sizeof(float));
            const uint32_t zero = 0u;
            if (c.terrainCount & 1u) s.add_host(&zero, 4);
        }
        s.add_dev(e->d_stencil, (size_t)c.stencilCount * sizeof(float4));
        out.push_back(std::move(s));
    }
    {
        StateSection s;
        s.tag = SPH_STATE_PARTICLES;
        s.add_dev(e->d_aos, e->n * sizeof(SphParticle));
        out.push_back(std::move(s));
    }
    if (e->trM) {
        StateSection s;
        s.tag = SPH_STATE_TRACERS;
        sph::StateTracers t;
        std::memset(&t, 0, sizeof(t));
        t.m = e->trM; t.integrator = (uint32_t)e->trIntegrator; t.history = e->trK; t.stride = e->trS;
        state_tracer_words(e->trSteps, e->trK, e->trS, t.state);       // (the device words: sph_state_save holds them against the device's)
        t.hostSteps = e->trSteps;
        s.add_host(&t, sizeof(t));
        s.add_dev(e->d_trRec, e->trM * sizeof(SphTracer));
        s.add_dev(e->d_trRing, (size_t)sph::state_tracer_slots(e->trSteps, e->trK, e->trS) * e->trM * sizeof(float4));
        out.push_back(std::move(s));
    }
    if (e->dfC) {
        // (the pool's size lies on the device: its state words, and the crest books, are read first -- a few hundred bytes, no array)
        StateSection s;
        s.tag = SPH_STATE_DIFFUSE;
        uint32_t w[sph::DF_WORDS + 2] = {0}, cw[sph::DFC_WORDS + 2] = {0};
        if (current) {
            HIP_TRY(hipMemcpyAsync(w, e->d_dfState, sph::DF_WORDS * 4u, hipMemcpyDeviceToHost, e->stream));
            if (e->d_dfCrState) HIP_TRY(hipMemcpyAsync(cw, e->d_dfCrState, sph::DFC_WORDS * 4u, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else {                                                      // (sizes: the count alone)
            HIP_TRY(hipMemcpyAsync(&w[sph::DF_ALIVE], e->d_dfState + sph::DF_ALIVE, 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
        sph::StateDiffuse d;
        std::memset(&d, 0, sizeof(d));
        d.cfg = e->dfCfg; d.crest = e->dfCrCfg;
        d.crestOn = e->dfCrOn ? 1u : 0u; d.hasCrestBooks = e->d_dfCrState ? 1u : 0u;
        d.stateWords = (uint32_t)sph::DF_WORDS; d.crestWords = (uint32_t)sph::DFC_WORDS;
        d.alive = std::min(w[sph::DF_ALIVE], e->dfC);
        s.add_host(&d, sizeof(d));
        s.add_host(w, (size_t)sph::state_pad8(sph::DF_WORDS * 4u));
        if (d.hasCrestBooks) s.add_host(cw, (size_t)sph::state_pad8(sph::DFC_WORDS * 4u));
        s.add_dev(e->d_dfPool, (size_t)d.alive * sizeof(SphDiffuse));
        out.push_back(std::move(s));
    }
    if (e->scK) {
        StateSection s;
        s.tag = SPH_STATE_SCALARS;
        sph::StateScalars c;
        std::memset(&c, 0, sizeof(c));
        c.channels = e->scK; c.hasCouple = e->d_cpTab.p ? 1u : 0u; c.accBytes = (uint32_t)sizeof(sph::CoupleAcc); c.steps = e->scSteps;
        if (current) {
            HIP_TRY(hipMemcpyAsync(&c.stateWord, e->d_scState, 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
        std::memcpy(c.coeffs, e->scCoeffs, sizeof(float) * 2 * (size_t)e->scK);
        std::memcpy(c.beta, e->cpTab.beta, sizeof(c.beta)); std::memcpy(c.ref, e->cpTab.ref, sizeof(c.ref));
        c.nSrc = e->cpTab.nSrc;
        std::memcpy(c.src, e->cpTab.src, sizeof(c.src));
        s.add_host(&c, sizeof(c));
        if ((rc = s.add_dev32(e, e->d_scVal, e->scN * (size_t)e->scK, current))) return rc;
        if (c.hasCouple) s.add_dev(e->d_cpAcc, sizeof(sph::CoupleAcc));
        out.push_back(std::move(s));
    }
    bool anyVolume = false;
    for (const auto& v : e->vols) anyVolume = anyVolume || v.d != nullptr;
    if (e->obsK || anyVolume) {
        StateSection s;
        s.tag = SPH_STATE_OBSTACLES;
        sph::StateObstacles o;
        std::memset(&o, 0, sizeof(o));
        o.count = e->obsK; o.recBytes = (uint32_t)sizeof(sph::ObsRec); o.dynBytes = (uint32_t)sizeof(sph::ObsDyn); o.accBytes = (uint32_t)sizeof(sph::ObsAcc);
        for (int i = 0; i < sph::kObsMax; ++i) {
            o.bind[i] = i < e->obsK ? e->volTab.bind[i] : -1;
            if (i >= e->obsK) continue;
            o.shape[i] = e->obsShape[i];
            o.dynOn[i] = e->dynOn[i] ? 1 : 0;
            if (e->dynOn[i]) o.dynSet[i] = e->dynSet[i];
        }
        for (int i = 0; i < sph::kVolMax; ++i)
            if (e->vols[i].d) for (int a = 0; a < 3; ++a) { o.vol[i].dims[a] = e->vols[i].dims[a]; o.vol[i].spacing[a] = e->vols[i].spacing[a]; }
        s.add_host(&o, sizeof(o));
        if (e->obsK) {
            s.add_dev(e->d_obs.p, sizeof(sph::ObsRec) * (size_t)e->obsK);
            s.add_dev(e->d_obsAcc, sizeof(sph::ObsAcc));
            s.add_dev(e->d_dyn.p, sizeof(sph::ObsDyn) * (size_t)e->obsK);
        }
        for (int i = 0; i < sph::kVolMax; ++i)
            if (e->vols[i].d && (rc = s.add_dev32(e, e->vols[i].d, (size_t)e->vols[i].dims[0] * e->vols[i].dims[1] * e->vols[i].dims[2], current))) return rc;
        out.push_back(std::move(s));
    }
    if (e->gtTab.count && e->d_gtTab.p) {
        StateSection s;
        s.tag = SPH_STATE_GATES;
        sph::StateGates g;
        std::memset(&g, 0, sizeof(g));
        g.count = e->gtTab.count; g.history = e->gtTab.history; g.stride = e->gtTab.stride;
        g.accWords = (uint32_t)(sizeof(sph::GateAcc) / 8); g.ringRowWords = (uint32_t)sph::kGateRingRow;
        std::memcpy(g.set, e->gtSet, sizeof(g.set));
        s.add_host(&g, sizeof(g));
        s.add_dev(e->d_gtAcc, sizeof(sph::GateAcc));
        s.add_dev(e->d_gtRing.p, (size_t)g.history * sph::kGateRingRow * 8u);
        out.push_back(std::move(s));
    }
    if (e->monCount) {
        StateSection s;
        s.tag = SPH_STATE_MONITORS;
        for (int i = 0; i < sph::kMonitorMax; ++i) {
            const MonitorSlot& m = e->mon[i];
            sph::StateMonitorSlot r;
            std::memset(&r, 0, sizeof(r));
            r.kind = m.kind;
            if (m.kind != SPH_MONITOR_NONE) {
                r.m = m.m; r.cfg = m.cfg;
                for (int a = 0; a < 3; ++a) { r.dims[a] = m.dims[a]; r.origin[a] = m.origin[a]; r.spacing[a] = m.spacing[a]; }
            }
            s.add_host(&r, sizeof(r));
        }
        for (int i = 0; i < sph::kMonitorMax; ++i) {
            const MonitorSlot& m = e->mon[i];
            if (m.kind == SPH_MONITOR_NONE) continue;
            s.add_dev(m.d_tab.p, sph::kStateMonitorCounters);
            if (m.kind == SPH_MONITOR_POINTS) s.add_dev(m.d_points.p, m.m * sizeof(float4));
            s.add_dev(m.d_rows.p, m.m * sizeof(sph::MonitorRow));
            s.add_dev(m.d_ring.p, (size_t)m.cfg.history * m.cfg.ringPoints * sizeof(SphSample));
            s.add_dev(m.d_times.p, (size_t)m.cfg.history * sizeof(double));
        }
        out.push_back(std::move(s));
    }
    return SPH_OK;
}

static size_t state_total_bytes(const std::vector<StateSection>& secs) {
    size_t at = sizeof(sph::StateHeader) + sizeof(sph::StateEntry) * secs.size();
    for (const StateSection& s : secs) at = sph::state_align16(at) + s.bytes();
    return sph::state_align16(at);
}

int sph_state_size(SphEngine* e, size_t* bytes) {
    if (!e || !bytes) return fail(SPH_ERR_ARG, "null argument");
    std::vector<StateSection> secs;
    int rc;
    if ((rc = state_collect(e, false, secs))) return rc;
    *bytes = state_total_bytes(secs);
    return SPH_OK;
}

int sph_state_save(SphEngine* e, void* blob, size_t cap, size_t* written) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    std::vector<StateSection> secs;
    int rc;
    if ((rc = state_collect(e, true, secs))) return rc;
    const size_t total = state_total_bytes(secs);
    if (written) *written = total;
    if (cap < total) return fail(SPH_ERR_CAPACITY, "a checkpoint of %zu bytes (capacity %zu)", total, cap);
    if (!blob) return fail(SPH_ERR_ARG, "null argument");
    unsigned char* b = static_cast<unsigned char*>(blob);
    std::memset(b, 0, total);
    std::vector<sph::StateEntry> table(secs.size());
    size_t at = sizeof(sph::StateHeader) + sizeof(sph::StateEntry) * secs.size();
    uint32_t mask = 0;
    for (size_t i = 0; i < secs.size(); ++i) {
        at = sph::state_align16(at);
        table[i] = sph::StateEntry{secs[i].tag, 1u, at, secs[i].bytes(), {0, 0}};
        for (const StatePiece& p : secs[i].pieces) {
            if (p.dev) HIP_TRY(hipMemcpyAsync(b + at, p.dev, p.bytes, hipMemcpyDeviceToHost, e->stream));
            else std::memcpy(b + at, p.host.data(), p.bytes);
            at += p.bytes;
        }
        mask |= secs[i].tag;
    }
    uint32_t trWords[3] = {0, 0, 0};
    if (e->trM) HIP_TRY(hipMemcpyAsync(trWords, e->d_trState, sizeof(trWords), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->trM) {
        uint32_t want[3];
        state_tracer_words(e->trSteps, e->trK, e->trS, want);
        if (std::memcmp(want, trWords, sizeof(want)) != 0)
            return fail(SPH_ERR_STATE, "the tracers' device step counter (%u, %u, slot %u) is not the host mirror's (%llu substeps)", trWords[0], trWords[1], trWords[2],
                        (unsigned long long)e->trSteps);
    }
    for (sph::StateEntry& s : table) sph::state_checksum(b + s.offset, (size_t)s.bytes, 0, s.sum);
    std::memcpy(b + sizeof(sph::StateHeader), table.data(), sizeof(sph::StateEntry) * table.size());
    sph::StateHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = sph::kStateMagic; h.format = sph::kStateFormat; h.abi = (uint32_t)SPH_ABI_VERSION; h.checksumKind = SPH_STATE_CHECKSUM_MIX64;
    h.sectionCount = (uint32_t)secs.size(); h.n = e->n; h.totalBytes = total; h.sectionMask = mask; h.headerBytes = (uint32_t)sizeof(h);
    h.params = e->params;
    sph::state_checksum(&h, sph::kStateHeaderSummed, 0, h.sum);
    sph::state_checksum(table.data(), sizeof(sph::StateEntry) * table.size(), sph::kStateHeaderSummed / 8, h.sum);
    std::memcpy(b, &h, sizeof(h));
    return SPH_OK;
}

int sph_state_peek(const void* blob, size_t bytes, SphStateInfo* out) {
    if (!out) return fail(SPH_ERR_ARG, "null argument");
    char why[400];
    if (sph::state_parse(blob, bytes, out, why, sizeof(why)) != SPH_OK) return fail(SPH_ERR_ARG, "checkpoint blob: %s", why);
    return SPH_OK;
}

int sph_state_checksum_host(const void* bytes, size_t n, uint64_t out[2]) {
    if ((!bytes && n) || !out) return fail(SPH_ERR_ARG, "null argument");
    if (n % 8u) return fail(SPH_ERR_ARG, "%zu bytes are not a multiple of 8", n);
    out[0] = out[1] = 0;
    sph::state_checksum(bytes, n, 0, out);
    return SPH_OK;
}

int sph_state_digest(SphEngine* e, uint32_t sections, SphStateDigest* out) {
    if (!e || !out) return fail(SPH_ERR_ARG, "null argument");
    if (sections & ~sph::kStateKnownMask) return fail(SPH_ERR_ARG, "unknown section bits %u", sections & ~sph::kStateKnownMask);
    std::vector<StateSection> secs;
    int rc;
    if ((rc = state_collect(e, true, secs))) return rc;
    if ((rc = e->d_stateAcc.grow(e, 2 * sph::kStateSections))) return rc;
    // the sums start at what the host's pieces add; the kernels add the device's pieces, each at its word index inside the section
    uint64_t init[sph::kStateSections][2];
    std::memset(init, 0, sizeof(init));
    uint32_t done = 0;
    for (const StateSection& s : secs) {
        if (sections && !(sections & s.tag)) continue;
        const int idx = sph::state_section_index(s.tag);
        size_t at = 0;
        for (const StatePiece& p : s.pieces) {
            if (!p.dev) sph::state_checksum(p.host.data(), p.bytes, at / 8, init[idx]);
            else if (((uintptr_t)p.dev & 15u) || (p.bytes & 7u)) return fail(SPH_ERR_STATE, "a piece of section %s is not 16-byte aligned", sph::state_section_name(s.tag));
            at += p.bytes;
        }
        done |= s.tag;
    }
    HIP_TRY(hipMemcpyAsync(e->d_stateAcc.p, init, sizeof(init), hipMemcpyHostToDevice, e->stream));
    for (const StateSection& s : secs) {
        if (!(done & s.tag)) continue;
        const int idx = sph::state_section_index(s.tag);
        size_t at = 0;
        for (const StatePiece& p : s.pieces) {
            if (p.dev) {
                const unsigned long long words = p.bytes / 8;
                Timed t(e, SPH_K_OTHER);
                hipLaunchKernelGGL(sph::k_state_checksum, dim3(sph::state_checksum_blocks(words)), dim3(sph::kStateBlock), 0, e->stream,
                                   static_cast<const unsigned long long*>(p.dev), words, (unsigned long long)(at / 8), e->d_stateAcc.p + 2 * idx);
            }
            at += p.bytes;
        }
    }
    HIP_TRY(hipGetLastError());
    std::memset(out, 0, sizeof(*out));
    HIP_TRY(hipMemcpyAsync(out->sum, e->d_stateAcc.p, sizeof(out->sum), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < sph::kStateSections; ++i) if (!(done & (1u << i))) out->sum[i][0] = out->sum[i][1] = 0;
    out->sections = done;
    return SPH_OK;
}

// What a load checks of the sections' configs beyond state_parse, by the checks of the set calls, before the engine is touched.
static int state_load_check(SphEngine* e, const unsigned char* b, const SphStateInfo& info) {
    int rc;
    if ((rc = validate_params(info.params))) return rc;
    sph::StateCore c;
    std::memcpy(&c, b + info.offset[0], sizeof(c));
    if (c.terrainCount) {
        if ((rc = validate_river(c.river))) return rc;
        for (uint64_t i = 0; i < c.terrainCount; ++i) {
            float v;
            std::memcpy(&v, b + info.offset[0] + sizeof(c) + 4 * i, 4);
            if (!std::isfinite(v)) return fail(SPH_ERR_ARG, "checkpoint blob: terrain height %llu is not finite", (unsigned long long)i);
        }
    }
    if (info.sections & SPH_STATE_TRACERS) {
        sph::StateTracers t;
        std::memcpy(&t, b + info.offset[2], sizeof(t));
        if ((rc = tracers_check(e, reinterpret_cast<const float*>(b), (size_t)t.m, (int)t.integrator, t.history, t.stride))) return rc;
        uint32_t want[3];
        state_tracer_words(t.hostSteps, t.history, t.stride, want);
        if (std::memcmp(want, t.state, sizeof(want)) != 0) return fail(SPH_ERR_ARG, "checkpoint blob: the tracers' device words do not belong to %llu substeps", (unsigned long long)t.hostSteps);
    }
    if (info.sections & SPH_STATE_DIFFUSE) {
        if ((rc = needs_sorted_copy(e, "diffuse particles need"))) return rc;
        sph::StateDiffuse d;
        std::memcpy(&d, b + info.offset[3], sizeof(d));
        if ((rc = diffuse_check_config(d.cfg))) return rc;
        if (d.stateWords != (uint32_t)sph::DF_WORDS || d.crestWords != (uint32_t)sph::DFC_WORDS)
            return fail(SPH_ERR_ARG, "checkpoint blob: a diffuse pool of %u + %u state words (this build: %d + %d)", d.stateWords, d.crestWords, sph::DF_WORDS, sph::DFC_WORDS);
        uint32_t alive;
        std::memcpy(&alive, b + info.offset[3] + sizeof(d) + 4 * sph::DF_ALIVE, 4);
        if (std::min(alive, d.cfg.capacity) != d.alive) return fail(SPH_ERR_ARG, "checkpoint blob: the diffuse pool's state words count %u living records, the section holds %u", alive, d.alive);
        if (d.crestOn) {
            SphGridInfo g;
            sph::compute_grid_extents(info.params, g);
            if ((rc = diffuse_check_crest(d.crest, info.params.param_h, g.cellSize))) return rc;
        }
    }
    if (info.sections & SPH_STATE_SCALARS) {
        if ((rc = scalars_refused(e))) return rc;
        sph::StateScalars c;
        std::memcpy(&c, b + info.offset[4], sizeof(c));
        if ((rc = scalars_check_coeffs(c.coeffs, c.channels)) || (rc = couple_check_buoyancy(c.beta, c.ref, c.channels)) ||
            (rc = couple_check_sources(c.src, c.nSrc, c.channels))) return rc;
        if (c.hasCouple && c.accBytes != sizeof(sph::CoupleAcc)) return fail(SPH_ERR_ARG, "checkpoint blob: injected books of %u bytes (this build: %zu)", c.accBytes, sizeof(sph::CoupleAcc));
    }
    if (info.sections & SPH_STATE_OBSTACLES) {
        std::unique_ptr<sph::StateObstacles> o(new sph::StateObstacles());
        std::memcpy(o.get(), b + info.offset[5], sizeof(*o));
        if (o->recBytes != sizeof(sph::ObsRec) || o->dynBytes != sizeof(sph::ObsDyn) || o->accBytes != sizeof(sph::ObsAcc))
            return fail(SPH_ERR_ARG, "checkpoint blob: body records of %u / %u bytes and sums of %u (this build: %zu / %zu and %zu)", o->recBytes, o->dynBytes, o->accBytes,
                        sizeof(sph::ObsRec), sizeof(sph::ObsDyn), sizeof(sph::ObsAcc));
        SphObstacle obs[sph::kObsMax];
        for (int i = 0; i < o->count; ++i) {
            sph::ObsRec r;
            std::memcpy(&r, b + info.offset[5] + sizeof(*o) + sizeof(r) * i, sizeof(r));
            rec_to_obstacle(r, obs[i]);
            if (r.shape != o->shape[i]) return fail(SPH_ERR_ARG, "checkpoint blob: body %d has shape %d in its record and %d in the table", i, r.shape, o->shape[i]);
            if (o->bind[i] >= 0 && r.shape != SPH_OBSTACLE_BOX) return fail(SPH_ERR_ARG, "checkpoint blob: body %d is bound to a volume and is not a box", i);
            sph::ObsDyn dr;
            if (o->dynOn[i] && (rc = dynamics_to_rec(o->dynSet[i], i, dr))) return rc;
        }
        if ((rc = obstacles_check(obs, o->count))) return rc;
        for (int i = 0; i < sph::kVolMax; ++i)
            if (sph::state_volume_points(o->vol[i]) > 0 && (rc = check_lattice(o->vol[i].dims, o->vol[i].spacing, 2, nullptr))) return rc;
    }
    if (info.sections & SPH_STATE_GATES) {
        if ((rc = needs_sorted_copy(e, "gates need"))) return rc;
        sph::StateGates g;
        std::memcpy(&g, b + info.offset[6], sizeof(g));
        if ((rc = gates_check(g.set, g.count))) return rc;
        if (g.stride == 0) return fail(SPH_ERR_ARG, "checkpoint blob: gate stride must be >= 1");
        if (g.accWords != sizeof(sph::GateAcc) / 8 || g.ringRowWords != (uint32_t)sph::kGateRingRow)
            return fail(SPH_ERR_ARG, "checkpoint blob: gate books of %u words and ring rows of %u (this build: %zu and %d)", g.accWords, g.ringRowWords,
                        sizeof(sph::GateAcc) / 8, sph::kGateRingRow);
    }
    if (info.sections & SPH_STATE_MONITORS) {
        if ((rc = monitor_refused(e))) return rc;
        for (int i = 0; i < sph::kMonitorMax; ++i) {
            sph::StateMonitorSlot s;
            std::memcpy(&s, b + info.offset[7] + sizeof(s) * i, sizeof(s));
            if (s.kind == SPH_MONITOR_NONE) continue;
            SphMonitorConfig cfg;
            if ((rc = monitor_config_check(&s.cfg, (size_t)s.m, &cfg))) return rc;
            if (std::memcmp(&cfg, &s.cfg, sizeof(cfg)) != 0) return fail(SPH_ERR_ARG, "checkpoint blob: monitor %d does not carry the config in force", i);
            if (s.kind == SPH_MONITOR_LATTICE) {
                long long total = 0;
                if ((rc = check_lattice(s.dims, s.spacing, 1, &total))) return rc;
                if ((uint64_t)total != s.m || !obs_all_finite(s.origin, 3)) return fail(SPH_ERR_ARG, "checkpoint blob: monitor %d's lattice does not have its %llu points", i, (unsigned long long)s.m);
            }
        }
    }
    return SPH_OK;
}

int sph_state_load(SphEngine* e, const void* blob, size_t bytes) {
    if (!e) return fail(SPH_ERR_ARG, "null engine");
    if (e->slab) return fail(SPH_ERR_STATE, "checkpoints of a z-slab engine are not supported: its state is one share of a decomposed run");
    SphStateInfo info;
    int rc;
    if ((rc = sph_state_peek(blob, bytes, &info))) return rc;
    const unsigned char* b = static_cast<const unsigned char*>(blob);
    if ((rc = state_load_check(e, b, info))) return rc;

    // ---- from here on the engine changes ----
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->surfValid = false;                                             // query results: "no result", as after sph_reset
    neighbors_free(e); components_free(e); knn_free(e); rays_free(e); shell_free(e); aniso_free(e); aggregate_free(e);
    tracers_free(e); diffuse_free(e); scalars_free(e); gates_free(e); monitors_free(e);
    obstacles_free(e); volumes_free(e);
    for (auto& s : e->obsShape) s = 0;
    for (auto& d : e->dynSet) d = SphObstacleDynamics{};

    sph::StateCore c;
    std::memcpy(&c, b + info.offset[0], sizeof(c));
    const unsigned char* tail = b + info.offset[0] + sizeof(c);
    e->params = c.params;
    e->lastDt = c.lastDt;
    e->fountain = c.fountain;
    if (c.terrainCount) {
        std::vector<float> heights(c.terrainCount);
        std::memcpy(heights.data(), tail, 4 * c.terrainCount);
        e->terrainHeights.clear();                                    // (another heightfield size than the engine's is no error here)
        if ((rc = sph_set_river(e, &c.river, heights.data()))) return rc;
    } else {
        e->terrainHeights.clear();
        e->river = c.river;
    }
    tail += (4 * c.terrainCount + 7u) & ~(uint64_t)7u;
    {
        std::vector<float> pts(4 * c.stencilCount);
        if (c.stencilCount) std::memcpy(pts.data(), tail, 16 * c.stencilCount);
        if ((rc = sph_set_stencil_targets(e, pts.data(), (size_t)c.stencilCount))) return rc;
    }
    sph::compute_grid_extents(e->params, e->grid);
    free_particle_buffers(e);                                         // (the graph cache goes with them)
    {
        std::vector<SphParticle> rec(info.n);
        std::memcpy(rec.data(), b + info.offset[1], info.n * sizeof(SphParticle));
        if ((rc = set_particles(e, rec.data(), rec.size())) || (rc = ensure_grid_buffers(e))) return rc;
    }

    if (info.sections & SPH_STATE_OBSTACLES) {                        // (in front of the scalars: a source may ride on a body)
        const unsigned char* p = b + info.offset[5];
        std::unique_ptr<sph::StateObstacles> o(new sph::StateObstacles());
        std::memcpy(o.get(), p, sizeof(*o));
        const unsigned char* recs = p + sizeof(*o);
        const unsigned char* acc = recs + sizeof(sph::ObsRec) * (size_t)o->count;
        const unsigned char* dyn = acc + (o->count ? sizeof(sph::ObsAcc) : 0);
        const unsigned char* vals = dyn + sizeof(sph::ObsDyn) * (size_t)o->count;
        if (o->count) {
            SphObstacle obs[sph::kObsMax];
            for (int i = 0; i < o->count; ++i) {
                sph::ObsRec r;
                std::memcpy(&r, recs + sizeof(r) * i, sizeof(r));
                rec_to_obstacle(r, obs[i]);
            }
            if ((rc = sph_obstacles_set(e, obs, o->count))) return rc;
            for (int i = 0; i < o->count; ++i)
                if (o->dynOn[i] && (rc = sph_obstacles_set_dynamics(e, i, &o->dynSet[i]))) return rc;
        }
        for (int i = 0; i < sph::kVolMax; ++i) {                      // (every volume in the slot it had: the bindings name slots)
            const long long pts = sph::state_volume_points(o->vol[i]);
            if (pts <= 0) continue;
            int unused = -1;
            float* d = nullptr;
            if ((rc = volume_free_slot(e, &unused)) || (rc = dev_alloc(&d, (size_t)pts))) return rc;
            const hipError_t er = hipMemcpyAsync(d, vals, (size_t)pts * sizeof(float), hipMemcpyHostToDevice, e->stream);
            if (er != hipSuccess) { dev_free(d); return fail(SPH_ERR_HIP, "volume upload: %s", hipGetErrorString(er)); }
            if ((rc = volume_adopt(e, i, d, o->vol[i].dims, o->vol[i].spacing))) return rc;
            vals += sph::state_pad8(4ull * (uint64_t)pts);
        }
        for (int i = 0; i < o->count; ++i)
            if (o->bind[i] >= 0 && (rc = sph_obstacles_bind_volume(e, i, o->bind[i]))) return rc;
        if (o->count) {                                               // the advanced poses, the sums and the device's dynamics records over what the set calls made
            HIP_TRY(hipMemcpyAsync(e->d_obs.p, recs, sizeof(sph::ObsRec) * (size_t)o->count, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(e->d_obsAcc, acc, sizeof(sph::ObsAcc), hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(e->d_dyn.p, dyn, sizeof(sph::ObsDyn) * (size_t)o->count, hipMemcpyHostToDevice, e->stream));
        }
    }
    if (info.sections & SPH_STATE_SCALARS) {
        const unsigned char* p = b + info.offset[4];
        sph::StateScalars c;
        std::memcpy(&c, p, sizeof(c));
        const size_t words = (size_t)info.n * (size_t)c.channels;
        std::vector<float> values(words);
        std::memcpy(values.data(), p + sizeof(c), 4 * words);
        if ((rc = sph_scalars_set(e, values.data(), (size_t)info.n, c.channels, c.coeffs))) return rc;
        if (c.hasCouple) {
            SphScalarSource src[SPH_MAX_SCALAR_SOURCES];
            std::memcpy(src, c.src, sizeof(src));
            if ((rc = couple_ensure(e)) || (rc = sph_scalars_set_buoyancy(e, c.beta, c.ref)) || (rc = sph_scalars_set_sources(e, src, c.nSrc))) return rc;
            HIP_TRY(hipMemcpyAsync(e->d_cpAcc, p + sizeof(c) + sph::state_pad8(4ull * words), sizeof(sph::CoupleAcc), hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(hipMemcpyAsync(e->d_scState, p + offsetof(sph::StateScalars, stateWord), 4, hipMemcpyHostToDevice, e->stream));
        e->scSteps = c.steps;
    }
    if (info.sections & SPH_STATE_DIFFUSE) {
        const unsigned char* p = b + info.offset[3];
        sph::StateDiffuse d;
        std::memcpy(&d, p, sizeof(d));
        const unsigned char* words = p + sizeof(d);
        const unsigned char* crestWords = words + sph::state_pad8(4ull * sph::DF_WORDS);
        const unsigned char* pool = crestWords + (d.hasCrestBooks ? sph::state_pad8(4ull * sph::DFC_WORDS) : 0u);
        if ((rc = sph_diffuse_set(e, &d.cfg))) return rc;
        if (d.hasCrestBooks) {                                        // (the books exist once the term was on; off again: the books stay)
            SphDiffuseCrest on;
            sph_diffuse_crest_default(&on);
            if ((rc = sph_diffuse_set_crest(e, d.crestOn ? &d.crest : &on)) || (!d.crestOn && (rc = sph_diffuse_set_crest(e, nullptr)))) return rc;
            HIP_TRY(hipMemcpyAsync(e->d_dfCrState, crestWords, 4u * sph::DFC_WORDS, hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(hipMemcpyAsync(e->d_dfState, words, 4u * sph::DF_WORDS, hipMemcpyHostToDevice, e->stream));
        if (d.alive) HIP_TRY(hipMemcpyAsync(e->d_dfPool, pool, (size_t)d.alive * sizeof(SphDiffuse), hipMemcpyHostToDevice, e->stream));
    }
    if (info.sections & SPH_STATE_TRACERS) {
        const unsigned char* p = b + info.offset[2];
        sph::StateTracers t;
        std::memcpy(&t, p, sizeof(t));
        const unsigned char* recs = p + sizeof(t);
        std::vector<float> pts(4 * t.m);
        for (uint64_t i = 0; i < t.m; ++i) std::memcpy(&pts[4 * i], recs + 32 * i, 16);
        if ((rc = sph_tracers_set(e, pts.data(), (size_t)t.m, (int)t.integrator, t.history, t.stride))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_trRec, recs, 32 * t.m, hipMemcpyHostToDevice, e->stream));
        const uint64_t slots = sph::state_tracer_slots(t.hostSteps, t.history, t.stride);
        if (slots) HIP_TRY(hipMemcpyAsync(e->d_trRing, recs + 32 * t.m, 16ull * slots * t.m, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->d_trState, p + offsetof(sph::StateTracers, state), 12, hipMemcpyHostToDevice, e->stream));
        e->trSteps = t.hostSteps;
        e->trSorted = t.hostSteps;                                    // (not ordered yet: the next dispatch sorts)
    }
    if (info.sections & SPH_STATE_GATES) {
        const unsigned char* p = b + info.offset[6];
        sph::StateGates g;
        std::memcpy(&g, p, sizeof(g));
        if ((rc = sph_gates_set(e, g.set, g.count, g.history, g.stride))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_gtAcc, p + sizeof(g), sizeof(sph::GateAcc), hipMemcpyHostToDevice, e->stream));
        if (g.history) HIP_TRY(hipMemcpyAsync(e->d_gtRing.p, p + sizeof(g) + sizeof(sph::GateAcc), 8ull * g.history * sph::kGateRingRow, hipMemcpyHostToDevice, e->stream));
    }
    if (info.sections & SPH_STATE_MONITORS) {
        const unsigned char* dir = b + info.offset[7];
        const unsigned char* p = dir + sizeof(sph::StateMonitorSlot) * sph::kMonitorMax;
        for (int i = 0; i < sph::kMonitorMax; ++i) {
            sph::StateMonitorSlot s;
            std::memcpy(&s, dir + sizeof(s) * i, sizeof(s));
            if (s.kind == SPH_MONITOR_NONE) continue;
            unsigned long long ca[2];
            double time;
            std::memcpy(ca, p, 16); std::memcpy(&time, p + 16, 8);
            p += sph::kStateMonitorCounters;
            if (s.kind == SPH_MONITOR_POINTS) {
                std::vector<float> pts(4 * s.m);
                std::memcpy(pts.data(), p, 16 * s.m);
                p += 16 * s.m;
                if ((rc = sph_monitor_set(e, i, pts.data(), (size_t)s.m, &s.cfg))) return rc;
            } else if ((rc = sph_monitor_set_lattice(e, i, s.origin, s.spacing, s.dims, &s.cfg))) return rc;
            MonitorSlot& m = e->mon[i];
            HIP_TRY(hipMemcpyAsync(m.d_rows.p, p, sizeof(sph::MonitorRow) * s.m, hipMemcpyHostToDevice, e->stream));
            p += sizeof(sph::MonitorRow) * s.m;
            const size_t ring = (size_t)s.cfg.history * s.cfg.ringPoints * sizeof(SphSample);
            if (ring) HIP_TRY(hipMemcpyAsync(m.d_ring.p, p, ring, hipMemcpyHostToDevice, e->stream));
            p += ring;
            if (s.cfg.history) HIP_TRY(hipMemcpyAsync(m.d_times.p, p, 8ull * s.cfg.history, hipMemcpyHostToDevice, e->stream));
            p += 8ull * s.cfg.history;
            sph::MonitorTab tab = m.tab;                              // the table of the set, with the saved counters and what follows from them
            tab.c = ca[0]; tab.a = ca[1]; tab.time = time;
            tab.act = sph::monitor_acts(tab.c, tab.every) ? 1u : 0u;
            tab.row = sph::monitor_row_of(tab.a, tab.history, tab.stride);
            if ((rc = m.d_tab.put(e, &tab))) return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SPH_OK;
}

}  // extern "C"
