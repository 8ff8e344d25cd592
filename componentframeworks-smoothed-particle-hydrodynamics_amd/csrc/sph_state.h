// sph_state.h -- checkpoints: the blob format, its checksum (host and device) and the parser of untrusted blobs (no reference
// counterpart; DESIGN.md section 3t, include/sph_abi.h "checkpoints").
//
// Feature layer; it includes base headers only.  Everything above the __HIPCC__ guard is plain host C++ (it compiles with g++ or
// clang++ without HIP): the layout records, state_checksum() and state_parse().  state_parse() is the one piece of the engine that
// reads untrusted bytes: sph_state_peek is that function, and sph_state_load runs it before it touches the engine.
//
// The blob (little-endian):
//   StateHeader (256 bytes)  magic, format version, sph_abi_version(), checksum kind, section count, n, total bytes, the mask of the
//                            sections present, the SphParams of the saved engine, zeros, and the checksum of the header's first 240
//                            bytes and of the section table (word indices continue from the header into the table)
//   StateEntry[count]        tag (one bit of the mask), section version, offset, bytes, checksum of the payload (word index 0 at `offset`)
//   payloads                 in the table's order, each at the next multiple of 16 behind the one before, padded with zeros; the blob
//                            ends at the multiple of 16 behind the last payload.  The layout is canonical: every byte of a blob is
//                            either covered by a checksum or checked to be zero.
//
// The checksum of a byte range (a multiple of 8 bytes) read as little-endian 64-bit words w_i, i counted from a base word index:
//   lane L = sum over i of mix64(w_i + C_L + (base + i) * G)  mod 2^64,   L = 0, 1
// mix64 is the splitmix64 finaliser (a bijection of 64-bit words), G the golden-ratio odd constant, C_0 != C_1.  The terms are keyed by
// the word index (swapping two different records changes the sums); the sums commute (any evaluation order, any split into pieces: the
// checksum of a concatenation is the sum of the pieces' checksums at their base indices).  An integrity check, NOT a cryptographic
// hash: anyone can construct two blobs with the same sums.
//
//   k_state_checksum   streams 64-bit words of device memory (16-byte loads, grid-stride), sums the two lanes per wave (wave_sum, integer:
//                      any order gives the same bits), per block through LDS, and adds one 64-bit atomic per lane and block to acc[0..1]
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sph_abi.h"

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the checkpoint blob is little-endian and so must the host be"
#endif

#if defined(__HIPCC__)
#define SPH_STATE_HD __host__ __device__
#else
#define SPH_STATE_HD
#endif

namespace sph {

constexpr uint64_t kStateMagic = 0x4554415453485053ull;            // "SPHSTATE"
constexpr uint32_t kStateFormat = SPH_STATE_FORMAT;
constexpr uint64_t kStateGolden = 0x9e3779b97f4a7c15ull;
constexpr uint64_t kStateLane0 = 0x243f6a8885a308d3ull, kStateLane1 = 0x13198a2e03707344ull;
constexpr int kStateSections = SPH_STATE_SECTION_COUNT;
constexpr size_t kStateHeaderSummed = 240;                          // bytes of the header its own checksum covers

// ---- the checksum, stated once for host and device ------------------------------------------------------------
SPH_STATE_HD inline uint64_t state_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// The two terms of word w at word index `index`, added to s0 / s1.
SPH_STATE_HD inline void state_term(uint64_t w, uint64_t index, uint64_t& s0, uint64_t& s1) {
    const uint64_t k = w + index * kStateGolden;
    s0 += state_mix64(k + kStateLane0);
    s1 += state_mix64(k + kStateLane1);
}
// Host: adds the checksum of `bytes` bytes (a multiple of 8; any alignment) at word index `base` to out[0..1].
inline void state_checksum(const void* data, size_t bytes, uint64_t base, uint64_t out[2]) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint64_t s0 = 0, s1 = 0;
    for (size_t i = 0; i < bytes / 8; ++i) {
        uint64_t w;
        memcpy(&w, p + 8 * i, 8);
        state_term(w, base + i, s0, s1);
    }
    out[0] += s0; out[1] += s1;
}

// ---- the layout records (no padding: every field is naturally aligned) ----------------------------------------
struct StateHeader {
    uint64_t magic;
    uint32_t format, abi, checksumKind, sectionCount;
    uint64_t n, totalBytes;
    uint32_t sectionMask, headerBytes;
    SphParams params;
    unsigned char zero[kStateHeaderSummed - 48 - sizeof(SphParams)];
    uint64_t sum[2];
};
static_assert(sizeof(StateHeader) == 256 && offsetof(StateHeader, params) == 48 && offsetof(StateHeader, sum) == kStateHeaderSummed, "StateHeader is 256 bytes");
struct StateEntry {
    uint32_t tag, version;
    uint64_t offset, bytes;
    uint64_t sum[2];
};
static_assert(sizeof(StateEntry) == 40, "StateEntry is 40 bytes");

// CORE: this record, then terrainCount floats (padded with zeros to 8 bytes), then stencilCount float4.
struct StateCore {
    SphParams params;
    float lastDt;
    SphFountain fountain;
    SphRiver river;
    uint64_t terrainCount, stencilCount;
};
static_assert(sizeof(StateCore) == 280, "StateCore is 280 bytes");
// TRACERS: this record, then m 32-byte records in the caller's order, then the written slots of the pathline ring (state_tracer_slots()
// of them, in slot order, m float4 each: a slot no snapshot has reached yet holds nothing a call can return).
struct StateTracers {
    uint64_t m;
    uint32_t integrator, history, stride;
    uint32_t state[3];                                             // the device words: substeps low / high, the ring slot the next substep writes
    uint64_t hostSteps;                                            // the host mirror of the step counter
};
static_assert(sizeof(StateTracers) == 40, "StateTracers is 40 bytes");
// GATES: this record, then accWords 8-byte words of the books (device), then history * ringRowWords words of the ring.
struct StateGates {
    int32_t count;
    uint32_t history, stride;
    uint32_t accWords, ringRowWords, pad;
    SphGate set[SPH_MAX_GATES];
};
static_assert(sizeof(StateGates) == 24 + 64 * SPH_MAX_GATES, "StateGates layout");
// MONITORS: SPH_MAX_MONITORS of this record, then per slot that holds a monitor, in slot order: the counters (c, a, time: 24 bytes),
// the points (m float4, explicit points only), m 128-byte rows, history * ringPoints 32-byte samples, history doubles.
struct StateMonitorSlot {
    int32_t kind;
    uint32_t pad;
    uint64_t m;
    int32_t dims[3];
    float origin[3], spacing[3];
    SphMonitorConfig cfg;
    uint32_t pad2;
};
static_assert(sizeof(StateMonitorSlot) == 80 && sizeof(SphMonitorConfig) == 24, "StateMonitorSlot is 80 bytes");
constexpr size_t kStateMonitorCounters = 24;
// DIFFUSE: this record, then stateWords 32-bit state words of the pool (alive, substep counter, totals, class counts; padded to 8 bytes),
// then crestWords words of the crest books if hasCrestBooks (padded to 8), then the `alive` living records of 48 bytes in pool order.
struct StateDiffuse {
    SphDiffuseConfig cfg;
    SphDiffuseCrest crest;                                         // the crest config in force (all zero while off)
    uint32_t crestOn, hasCrestBooks, stateWords, crestWords;
    uint32_t alive, pad;
};
static_assert(sizeof(StateDiffuse) == 64 + 48 + 24, "StateDiffuse is 136 bytes");
// SCALARS: this record, then n * channels floats by particle id (padded to 8 bytes), then accBytes of the injected books if hasCouple.
struct StateScalars {
    int32_t channels;
    uint32_t hasCouple, accBytes, stateWord;                       // stateWord: the device word of the last substep's diffusion number
    uint64_t steps;
    float coeffs[2 * SPH_MAX_SCALAR_CHANNELS];
    float beta[SPH_MAX_SCALAR_CHANNELS], ref[SPH_MAX_SCALAR_CHANNELS];
    int32_t nSrc, pad[3];
    SphScalarSource src[SPH_MAX_SCALAR_SOURCES];
};
static_assert(sizeof(StateScalars) == 24 + 32 + 32 + 16 + 64 * SPH_MAX_SCALAR_SOURCES, "StateScalars layout");
// OBSTACLES: this record, then count device body records of recBytes (the advanced poses), accBytes of the impulse sums (count > 0),
// count device dynamics records of dynBytes, then per volume slot in use its dims[0] * dims[1] * dims[2] floats (padded to 8 bytes).
struct StateVolume { int32_t dims[3]; float spacing[3]; };        // dims all zero: the slot is empty
struct StateObstacles {
    int32_t count;
    uint32_t recBytes, dynBytes, accBytes;
    int32_t shape[SPH_MAX_OBSTACLES], dynOn[SPH_MAX_OBSTACLES], bind[SPH_MAX_OBSTACLES];
    SphObstacleDynamics dynSet[SPH_MAX_OBSTACLES];                 // the records as set (zero where the body is kinematic)
    StateVolume vol[SPH_MAX_VOLUMES];
};
static_assert(sizeof(StateObstacles) == 16 + 12 * SPH_MAX_OBSTACLES + 80 * SPH_MAX_OBSTACLES + 24 * SPH_MAX_VOLUMES, "StateObstacles layout");
inline uint64_t state_pad8(uint64_t v) { return (v + 7u) & ~(uint64_t)7u; }
// Points of a saved volume slot: 0 for an empty slot, -1 for dims no volume can have.
inline long long state_volume_points(const StateVolume& v) {
    if (v.dims[0] == 0 && v.dims[1] == 0 && v.dims[2] == 0) return 0;
    long long total = 1;
    for (int a = 0; a < 3; ++a) {
        if (v.dims[a] < 2) return -1;
        total *= v.dims[a];
        if (total > 2147483647ll) return -1;
    }
    return total;
}

// A history ring of `history` rows that has taken `taken` rows so far, row q into slot q mod history: the oldest row it still holds and
// how many it holds.  The one statement of the rule for the engine's three rings (pathlines, gate history, monitor history); it lives
// here because this is the host code that must also compile without HIP.
struct RingSpan { uint64_t first; uint32_t have; };
inline RingSpan ring_span(uint64_t taken, uint32_t history) {
    const uint32_t have = (uint32_t)(taken < history ? taken : history);
    return RingSpan{taken - have, have};
}

// The ring slots of the tracers' pathlines written so far: snapshot q (taken after q * stride substeps, 0 the seed) lies in slot q mod
// history, so after `steps` substeps the first `have` slots hold snapshots and the others were never written.
inline uint64_t state_tracer_slots(uint64_t steps, uint32_t history, uint32_t stride) {
    return (history && stride) ? ring_span(steps / stride + 1u, history).have : 0;
}

inline const char* state_section_name(uint32_t tag) {
    switch (tag) {
    case SPH_STATE_CORE: return "core";
    case SPH_STATE_PARTICLES: return "particles";
    case SPH_STATE_TRACERS: return "tracers";
    case SPH_STATE_DIFFUSE: return "diffuse";
    case SPH_STATE_SCALARS: return "scalars";
    case SPH_STATE_OBSTACLES: return "obstacles";
    case SPH_STATE_GATES: return "gates";
    case SPH_STATE_MONITORS: return "monitors";
    default: return "unknown";
    }
}
inline int state_section_index(uint32_t tag) {
    for (int i = 0; i < kStateSections; ++i) if (tag == (1u << i)) return i;
    return -1;
}
constexpr uint32_t kStateKnownMask = (1u << kStateSections) - 1u;

inline size_t state_align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// a * b + c without overflow; false: it does not fit `limit`.
inline bool state_mul_add(uint64_t a, uint64_t b, uint64_t c, uint64_t limit, uint64_t* out) {
    if (c > limit || (a != 0 && b > (limit - c) / a)) return false;
    *out = a * b + c;
    return true;
}

// The bytes a section's payload must have by its own config words, or false with a message.  `p` holds `bytes` bytes.
inline bool state_section_expected(uint32_t tag, const unsigned char* p, uint64_t bytes, uint64_t n, const SphParams& headerParams, uint64_t* want,
                                   char* err, size_t errCap) {
    const uint64_t lim = (uint64_t)1 << 62;
    const char* name = state_section_name(tag);
    auto fixed = [&](size_t need) {
        if (bytes >= need) return true;
        snprintf(err, errCap, "section %s has %llu bytes, less than its %zu-byte record", name, (unsigned long long)bytes, need);
        return false;
    };
    auto too_big = [&]() { snprintf(err, errCap, "section %s: the sizes its config names overflow", name); return false; };
    switch (tag) {
    case SPH_STATE_CORE: {
        if (!fixed(sizeof(StateCore))) return false;
        StateCore c;
        memcpy(&c, p, sizeof(c));
        if (memcmp(&c.params, &headerParams, sizeof(SphParams)) != 0) { snprintf(err, errCap, "section core: its params differ from the header's"); return false; }
        if (c.terrainCount != 0 && (c.river.terrainW < 2 || c.river.terrainH < 2 || c.river.terrainW > 4096 || c.river.terrainH > 4096 ||
                                    c.terrainCount != (uint64_t)c.river.terrainW * (uint64_t)c.river.terrainH)) {
            snprintf(err, errCap, "section core: %llu terrain heights for a heightfield of %d x %d", (unsigned long long)c.terrainCount, c.river.terrainW, c.river.terrainH);
            return false;
        }
        uint64_t t = (c.terrainCount * 4u + 7u) & ~(uint64_t)7u;
        if (!state_mul_add(c.stencilCount, 16, sizeof(StateCore) + t, lim, want)) return too_big();
        return true;
    }
    case SPH_STATE_PARTICLES:
        if (!state_mul_add(n, sizeof(SphParticle), 0, lim, want)) return too_big();
        return true;
    case SPH_STATE_TRACERS: {
        if (!fixed(sizeof(StateTracers))) return false;
        StateTracers t;
        memcpy(&t, p, sizeof(t));
        uint64_t ring = 0;
        if (t.m == 0 || t.m > 2147483647ull || t.stride == 0u || !state_mul_add(t.history, t.m, 0, 2147483647ull, &ring) ||
            !state_mul_add(state_tracer_slots(t.hostSteps, t.history, t.stride), t.m, 0, 2147483647ull, &ring)) {
            snprintf(err, errCap, "section tracers: %llu tracers with a history of %u", (unsigned long long)t.m, t.history);
            return false;
        }
        if (!state_mul_add(t.m, 32, sizeof(StateTracers) + ring * 16u, lim, want)) return too_big();
        return true;
    }
    case SPH_STATE_GATES: {
        if (!fixed(sizeof(StateGates))) return false;
        StateGates g;
        memcpy(&g, p, sizeof(g));
        if (g.count < 1 || g.count > SPH_MAX_GATES || g.history > SPH_MAX_GATE_HISTORY || g.accWords > 4096u || g.ringRowWords > 4096u) {
            snprintf(err, errCap, "section gates: %d gates, history %u, %u + %u words per table and ring row", g.count, g.history, g.accWords, g.ringRowWords);
            return false;
        }
        *want = sizeof(StateGates) + 8ull * g.accWords + 8ull * (uint64_t)g.history * g.ringRowWords;
        return true;
    }
    case SPH_STATE_MONITORS: {
        if (!fixed(sizeof(StateMonitorSlot) * SPH_MAX_MONITORS)) return false;
        uint64_t total = sizeof(StateMonitorSlot) * SPH_MAX_MONITORS;
        int held = 0;
        for (int i = 0; i < SPH_MAX_MONITORS; ++i) {
            StateMonitorSlot s;
            memcpy(&s, p + sizeof(StateMonitorSlot) * i, sizeof(s));
            if (s.kind == SPH_MONITOR_NONE) continue;
            ++held;
            if ((s.kind != SPH_MONITOR_POINTS && s.kind != SPH_MONITOR_LATTICE) || s.m == 0 || s.m > (uint64_t)SPH_MAX_MONITOR_POINTS ||
                s.cfg.history > SPH_MAX_MONITOR_HISTORY || s.cfg.ringPoints > s.m) {
                snprintf(err, errCap, "section monitors: slot %d has kind %d, %llu points, history %u, %u ring points", i, s.kind, (unsigned long long)s.m,
                         s.cfg.history, s.cfg.ringPoints);
                return false;
            }
            total += kStateMonitorCounters + (s.kind == SPH_MONITOR_POINTS ? 16u * s.m : 0u) + sizeof(SphMonitorRow) * s.m +
                     (uint64_t)s.cfg.history * s.cfg.ringPoints * sizeof(SphSample) + 8ull * s.cfg.history;
        }
        if (!held) { snprintf(err, errCap, "section monitors holds no monitor"); return false; }
        *want = total;
        return true;
    }
    case SPH_STATE_DIFFUSE: {
        if (!fixed(sizeof(StateDiffuse))) return false;
        StateDiffuse d;
        memcpy(&d, p, sizeof(d));
        if (d.cfg.capacity == 0u || d.cfg.capacity > 2147483647u || d.alive > d.cfg.capacity || d.stateWords > 1024u || d.crestWords > 1024u ||
            d.crestOn > 1u || d.hasCrestBooks > 1u || (d.crestOn && !d.hasCrestBooks)) {
            snprintf(err, errCap, "section diffuse: %u living records for a capacity of %u, %u + %u state words", d.alive, d.cfg.capacity, d.stateWords, d.crestWords);
            return false;
        }
        *want = sizeof(StateDiffuse) + state_pad8(4ull * d.stateWords) + (d.hasCrestBooks ? state_pad8(4ull * d.crestWords) : 0u) + (uint64_t)d.alive * sizeof(SphDiffuse);
        return true;
    }
    case SPH_STATE_SCALARS: {
        if (!fixed(sizeof(StateScalars))) return false;
        StateScalars c;
        memcpy(&c, p, sizeof(c));
        if (c.channels < 1 || c.channels > SPH_MAX_SCALAR_CHANNELS || c.nSrc < 0 || c.nSrc > SPH_MAX_SCALAR_SOURCES || c.hasCouple > 1u || c.accBytes > 65536u ||
            (c.accBytes & 7u) || (c.nSrc && !c.hasCouple)) {
            snprintf(err, errCap, "section scalars: %d channels, %d sources, books of %u bytes", c.channels, c.nSrc, c.accBytes);
            return false;
        }
        *want = sizeof(StateScalars) + state_pad8(4ull * n * (uint64_t)c.channels) + (c.hasCouple ? c.accBytes : 0u);
        return true;
    }
    case SPH_STATE_OBSTACLES: {
        if (!fixed(sizeof(StateObstacles))) return false;
        StateObstacles o;
        memcpy(&o, p, sizeof(o));
        if (o.count < 0 || o.count > SPH_MAX_OBSTACLES || o.recBytes > 4096u || o.dynBytes > 4096u || o.accBytes > 65536u || ((o.recBytes | o.dynBytes | o.accBytes) & 7u)) {
            snprintf(err, errCap, "section obstacles: %d bodies, records of %u and %u bytes, sums of %u", o.count, o.recBytes, o.dynBytes, o.accBytes);
            return false;
        }
        uint64_t total = sizeof(StateObstacles) + (uint64_t)o.count * (o.recBytes + o.dynBytes) + (o.count ? o.accBytes : 0u);
        bool any = o.count > 0;
        for (int i = 0; i < SPH_MAX_VOLUMES; ++i) {
            const long long pts = state_volume_points(o.vol[i]);
            if (pts < 0) { snprintf(err, errCap, "section obstacles: volume %d has dims %d x %d x %d", i, o.vol[i].dims[0], o.vol[i].dims[1], o.vol[i].dims[2]); return false; }
            any = any || pts > 0;
            total += state_pad8(4ull * (uint64_t)pts);
        }
        for (int i = 0; i < SPH_MAX_OBSTACLES; ++i) {
            const int b = o.bind[i];
            if (b < -1 || b >= SPH_MAX_VOLUMES || (b >= 0 && (i >= o.count || state_volume_points(o.vol[b]) <= 0))) {
                snprintf(err, errCap, "section obstacles: body %d is bound to volume %d, which the section does not hold", i, b);
                return false;
            }
        }
        if (!any) { snprintf(err, errCap, "section obstacles holds neither a body nor a volume"); return false; }
        *want = total;
        return true;
    }
    default:
        snprintf(err, errCap, "section %s (tag %u) is not supported by this build", name, tag);
        return false;
    }
}

// The parser and validator of a blob: magic, versions, the canonical layout, every size against its own config, every checksum,
// unknown tags.  Returns SPH_OK and fills *out, or SPH_ERR_ARG with a message in err.  Reads blob[0, bytes) only.
inline int state_parse(const void* blob, size_t bytes, SphStateInfo* out, char* err, size_t errCap) {
    char none[8];
    if (!err || !errCap) { err = none; errCap = sizeof(none); }
    err[0] = 0;
    if (!blob) { snprintf(err, errCap, "null blob"); return SPH_ERR_ARG; }
    const unsigned char* b = static_cast<const unsigned char*>(blob);
    if (bytes < sizeof(StateHeader)) { snprintf(err, errCap, "truncated blob: %zu bytes, the header alone has %zu", bytes, sizeof(StateHeader)); return SPH_ERR_ARG; }
    StateHeader h;
    memcpy(&h, b, sizeof(h));
    if (h.magic != kStateMagic) { snprintf(err, errCap, "wrong magic %016llx: not a checkpoint blob", (unsigned long long)h.magic); return SPH_ERR_ARG; }
    if (h.format != kStateFormat) { snprintf(err, errCap, "format version %u (this build reads %u)", h.format, kStateFormat); return SPH_ERR_ARG; }
    if (h.abi != (uint32_t)SPH_ABI_VERSION) { snprintf(err, errCap, "saved under ABI version %u (this build is %d)", h.abi, SPH_ABI_VERSION); return SPH_ERR_ARG; }
    if (h.checksumKind != (uint32_t)SPH_STATE_CHECKSUM_MIX64) { snprintf(err, errCap, "unknown checksum kind %u", h.checksumKind); return SPH_ERR_ARG; }
    if (h.headerBytes != sizeof(StateHeader)) { snprintf(err, errCap, "header of %u bytes (expected %zu)", h.headerBytes, sizeof(StateHeader)); return SPH_ERR_ARG; }
    if (h.totalBytes > bytes) { snprintf(err, errCap, "truncated blob: %zu bytes of %llu", bytes, (unsigned long long)h.totalBytes); return SPH_ERR_ARG; }
    if (h.totalBytes < bytes) { snprintf(err, errCap, "%zu bytes given, the blob has %llu", bytes, (unsigned long long)h.totalBytes); return SPH_ERR_ARG; }
    if (h.n == 0) { snprintf(err, errCap, "n = 0: a checkpoint holds at least one particle"); return SPH_ERR_ARG; }
    if (h.n > ((uint64_t)1 << 30)) { snprintf(err, errCap, "n = %llu exceeds the engine limit", (unsigned long long)h.n); return SPH_ERR_ARG; }
    if (h.sectionCount == 0 || h.sectionCount > (uint32_t)kStateSections) { snprintf(err, errCap, "%u sections (1 .. %d)", h.sectionCount, kStateSections); return SPH_ERR_ARG; }
    const size_t tableEnd = sizeof(StateHeader) + sizeof(StateEntry) * (size_t)h.sectionCount;
    if (tableEnd > bytes) { snprintf(err, errCap, "truncated blob: the section table ends at %zu of %zu bytes", tableEnd, bytes); return SPH_ERR_ARG; }
    for (size_t i = 0; i < sizeof(h.zero); ++i)
        if (h.zero[i]) { snprintf(err, errCap, "reserved header byte %zu is not zero", 48 + sizeof(SphParams) + i); return SPH_ERR_ARG; }
    uint64_t hs[2] = {0, 0};
    state_checksum(b, kStateHeaderSummed, 0, hs);
    state_checksum(b + sizeof(StateHeader), tableEnd - sizeof(StateHeader), kStateHeaderSummed / 8, hs);
    if (hs[0] != h.sum[0] || hs[1] != h.sum[1]) { snprintf(err, errCap, "wrong checksum of the header and section table"); return SPH_ERR_ARG; }

    SphStateInfo info;
    memset(&info, 0, sizeof(info));
    info.formatVersion = h.format; info.abiVersion = h.abi; info.checksumKind = h.checksumKind;
    info.n = h.n; info.totalBytes = h.totalBytes; info.params = h.params;
    uint64_t end = tableEnd;                                           // where the payload before ends
    uint32_t mask = 0;
    for (uint32_t i = 0; i < h.sectionCount; ++i) {
        StateEntry s;
        memcpy(&s, b + sizeof(StateHeader) + sizeof(StateEntry) * (size_t)i, sizeof(s));
        const int idx = state_section_index(s.tag);
        if (idx < 0) { snprintf(err, errCap, "unknown section tag %u", s.tag); return SPH_ERR_ARG; }
        const char* name = state_section_name(s.tag);
        if (mask & s.tag) { snprintf(err, errCap, "section %s appears twice", name); return SPH_ERR_ARG; }
        if (mask > s.tag) { snprintf(err, errCap, "section %s is out of order", name); return SPH_ERR_ARG; }
        if (s.offset > h.totalBytes || s.bytes > h.totalBytes - s.offset) {
            snprintf(err, errCap, "section %s runs past the end of the blob (offset %llu, %llu bytes, blob %llu)", name, (unsigned long long)s.offset,
                     (unsigned long long)s.bytes, (unsigned long long)h.totalBytes);
            return SPH_ERR_ARG;
        }
        if (s.offset < end) { snprintf(err, errCap, "section %s at offset %llu overlaps what ends at %llu", name, (unsigned long long)s.offset, (unsigned long long)end); return SPH_ERR_ARG; }
        if (s.offset != state_align16(end)) { snprintf(err, errCap, "section %s at offset %llu, not at %llu", name, (unsigned long long)s.offset, (unsigned long long)state_align16(end)); return SPH_ERR_ARG; }
        if (s.bytes % 8u) { snprintf(err, errCap, "section %s has %llu bytes, not a multiple of 8", name, (unsigned long long)s.bytes); return SPH_ERR_ARG; }
        if (s.version != 1u) { snprintf(err, errCap, "section %s has version %u (this build reads 1)", name, s.version); return SPH_ERR_ARG; }
        for (uint64_t q = end; q < s.offset; ++q)
            if (b[q]) { snprintf(err, errCap, "padding byte %llu is not zero", (unsigned long long)q); return SPH_ERR_ARG; }
        uint64_t want = 0;
        if (!state_section_expected(s.tag, b + s.offset, s.bytes, h.n, h.params, &want, err, errCap)) return SPH_ERR_ARG;
        if (want != s.bytes) { snprintf(err, errCap, "section %s has %llu bytes, its config asks for %llu", name, (unsigned long long)s.bytes, (unsigned long long)want); return SPH_ERR_ARG; }
        uint64_t cs[2] = {0, 0};
        state_checksum(b + s.offset, (size_t)s.bytes, 0, cs);
        if (cs[0] != s.sum[0] || cs[1] != s.sum[1]) { snprintf(err, errCap, "wrong checksum of section %s", name); return SPH_ERR_ARG; }
        if (s.tag == SPH_STATE_CORE) {
            StateCore c;
            memcpy(&c, b + s.offset, sizeof(c));
            info.terrainCount = c.terrainCount; info.terrainOffset = c.terrainCount ? s.offset + sizeof(StateCore) : 0; info.stencilCount = c.stencilCount;
        }
        mask |= s.tag;
        info.offset[idx] = s.offset; info.bytes[idx] = s.bytes; info.version[idx] = s.version;
        info.sum[idx][0] = s.sum[0]; info.sum[idx][1] = s.sum[1];
        end = s.offset + s.bytes;
    }
    if (h.totalBytes != state_align16(end)) { snprintf(err, errCap, "the blob has %llu bytes, its sections end at %llu", (unsigned long long)h.totalBytes, (unsigned long long)state_align16(end)); return SPH_ERR_ARG; }
    for (uint64_t q = end; q < h.totalBytes; ++q)
        if (b[q]) { snprintf(err, errCap, "padding byte %llu is not zero", (unsigned long long)q); return SPH_ERR_ARG; }
    if (mask != h.sectionMask) { snprintf(err, errCap, "section mask %u, the table holds %u", h.sectionMask, mask); return SPH_ERR_ARG; }
    if ((mask & (SPH_STATE_CORE | SPH_STATE_PARTICLES)) != (SPH_STATE_CORE | SPH_STATE_PARTICLES)) { snprintf(err, errCap, "the core or the particles section is missing"); return SPH_ERR_ARG; }
    info.sections = mask;
    if (out) *out = info;
    return SPH_OK;
}

}  // namespace sph

// ---- device ----------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "sph_wave.h"

namespace sph {

constexpr int kStateBlock = 256;
constexpr int kStateGridMax = 2048;                                  // 256 CUs x 8 blocks; the rest is grid-strided

// words: 16-byte aligned; adds the checksum of words[0, count) at word index `base` to acc[0..1].
__global__ __launch_bounds__(kStateBlock) void k_state_checksum(const unsigned long long* __restrict__ words, unsigned long long count, unsigned long long base,
                                                                unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long sm[2 * (kStateBlock / 64)];
    const ulonglong2* __restrict__ pairs = reinterpret_cast<const ulonglong2*>(words);
    const unsigned long long nPairs = count >> 1;
    const unsigned long long stride = (unsigned long long)gridDim.x * kStateBlock;
    uint64_t s0 = 0, s1 = 0;
    unsigned long long i = (unsigned long long)blockIdx.x * kStateBlock + threadIdx.x;
    // two pairs per trip: both loads are issued before the first is hashed
    for (; i + stride < nPairs; i += 2 * stride) {
        const ulonglong2 a = pairs[i], b = pairs[i + stride];
        state_term(a.x, base + 2 * i, s0, s1);
        state_term(a.y, base + 2 * i + 1, s0, s1);
        state_term(b.x, base + 2 * (i + stride), s0, s1);
        state_term(b.y, base + 2 * (i + stride) + 1, s0, s1);
    }
    if (i < nPairs) {
        const ulonglong2 a = pairs[i];
        state_term(a.x, base + 2 * i, s0, s1);
        state_term(a.y, base + 2 * i + 1, s0, s1);
    }
    if ((count & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) state_term(words[count - 1], base + count - 1, s0, s1);
    s0 = wave_sum((unsigned long long)s0);
    s1 = wave_sum((unsigned long long)s1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[2 * w] = s0; sm[2 * w + 1] = s1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (int q = 0; q < kStateBlock / 64; ++q) t += sm[2 * q + threadIdx.x];
        atomicAdd(&acc[threadIdx.x], t);
    }
}

inline int state_checksum_blocks(unsigned long long count) {
    const unsigned long long pairs = (count >> 1) + 1ull;
    const unsigned long long b = (pairs + kStateBlock - 1) / kStateBlock;
    return (int)(b < (unsigned long long)kStateGridMax ? b : (unsigned long long)kStateGridMax);
}

}  // namespace sph
#endif
