// sph_slab.h -- the z-slab (multi-GPU) exchange (no reference counterpart; DESIGN.md section 8, include/sph_abi.h "z-slab decomposition").
// Included by sph_kernels.h, behind the substep's kernels.
//
// A slab engine owns the global cell layers [z0, z1) and keeps one ghost layer per side.  Per substep it packs what its neighbours need
// (k_slab_pack), the faces cross the links, and it appends what it received behind its own slots (k_slab_unpack*).  What the kernels and
// the host (sph_engine.hip, "z-slab entry points") share about that is stated here, once: the counter words (SlabCounter), the records
// per message (SlabMsg), the wire records and their sizes (SlabRec, HaloRec, SlabHdr, slab_*_msg_bytes, slab_face_*).  The flags: sph_device.h.
#pragma once
#include <stddef.h>
#include "sph_wave.h"   // wave_append

namespace sph {

// COUNTER WORDS: one device array of kSlabCounters words per engine (SphEngine::d_slabCnt, the kernels' `counters`), zero at creation
// but Live.  A lo / hi pair is adjacent: `name + d` is the word of direction d (0 = lo, 1 = hi).  Per word: who writes it; who resets it.
enum SlabCounter {
    kSlabCntRecLo, kSlabCntRecHi,          // k_slab_pack<false>: records appended per direction; sph_slab_pack zeroes them around its pack
    kSlabCntLive,                          // slots that hold data: sph_create_slab, every dispatch (the live count of its sort), k_slab_commit2 (+ received), sph_slab_unpack; never reset
    kSlabCntDownload,                      // k_slab_download: records written; sph_slab_download zeroes it before the launch
    kSlabCntFlags,                         // kSlabFlag* of sph_device.h, sticky: k_slab_headers2, k_slab_unpack*, k_slab_commit2, the SPH pass; sph_slab_clear_flags
    kSlabCntPackedLo, kSlabCntPackedHi,    // records per direction of the last pack, for sph_slab_status: k_slab_headers2, sph_slab_pack; sph_slab_pack zeroes them before its pack
    kSlabCntExchange,                      // k_slab_headers2: exchanges so far (goes into the headers); never reset
    kSlabCntHaloLo, kSlabCntHaloHi, kSlabCntMigLo, kSlabCntMigHi,                   // k_slab_pack<true>: running counts of the pack in flight; k_slab_headers2 zeroes them
    kSlabCntLastHaloLo, kSlabCntLastHaloHi, kSlabCntLastMigLo, kSlabCntLastMigHi,   // k_slab_headers2: the same four of the last pack, one SlabMsg (slab_note_counts reads it); never reset
    kSlabCounters
};
static_assert(kSlabCounters == 16, "16 counter words");

struct SlabMsg { uint32_t halo[2], mig[2]; };           // records per message: [0] to / from the lower neighbour, [1] the upper
static_assert(sizeof(SlabMsg) == 16 && offsetof(SlabMsg, mig) == 8 && kSlabCntLastMigLo - kSlabCntLastHaloLo == 2 && kSlabCntMigLo - kSlabCntHaloLo == 2,
              "the Last* counter words are a SlabMsg");

// 64-byte record that crosses ranks: a migrant (flags without F_HALO: the receiver owns it)
// or a boundary-layer copy (F_HALO set: candidate only).  acc travels too: a migrant's record of THIS substep
// (the 80-byte contract includes acc) is complete on its new owner even though the new owner never computed it.
struct SlabRec {
    float px, py, pz, vx, vy, vz, rho, prs, foam;
    uint32_t id, flags, pad;
    float ax, ay, az, pad2;
};
static_assert(sizeof(SlabRec) == 64, "SlabRec is 64 bytes");

__global__ __launch_bounds__(kBlock) void k_slab_import(const SphParticle* __restrict__ aos, const uint32_t* __restrict__ ids,
                                                        float4* __restrict__ pos, float4* __restrict__ vel, float2* __restrict__ rp,
                                                        float* __restrict__ foam, int n) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4* rec = reinterpret_cast<const float4*>(aos + i);
    float4 p = rec[0], v = rec[1], d = rec[3];
    int4 fl = *reinterpret_cast<const int4*>(rec + 4);
    uint32_t flags = (fl.x == 1 ? F_GHOST1 : 0u) | (fl.x != 0 ? F_GHOSTNZ : 0u) | (fl.y == 0 ? F_INACTIVE : 0u);
    pos[i] = make_float4(p.x, p.y, p.z, bitsf(flags));
    vel[i] = make_float4(v.x, v.y, v.z, bitsf(ids[i]));
    rp[i] = make_float2(d.x, d.y);
    foam[i] = d.z;
}

// Halo copies travel as 40-byte HaloRec (what a candidate needs: position, velocity, density, pressure, id, flags), only migrants
// as full 64-byte records.
struct HaloRec {
    float px, py, pz, vx, vy, vz, rho, prs;
    uint32_t id, flags;
};
static_assert(sizeof(HaloRec) == 40, "HaloRec is 40 bytes");
struct SlabHdr {                                        // first 64 bytes of a face buffer / of the migrant message
    uint32_t magic, nHalo, nHaloTrue, nMig, nMigTrue, exchange;
    uint32_t msgHalo, msgMig;                           // records the SENDER's two messages of this exchange carry (the receiver compares them with what it sized its receives for: kSlabFlagSizeMismatch)
    uint32_t pad[8];
};
static_assert(sizeof(SlabHdr) == 64, "SlabHdr is 64 bytes");
// The two messages per direction and exchange: header + the migrants in use, and the halo copies in use.
__host__ __device__ __forceinline__ size_t slab_mig_msg_bytes(size_t n) { return sizeof(SlabHdr) + n * sizeof(SlabRec); }
__host__ __device__ __forceinline__ size_t slab_halo_msg_bytes(size_t n) { return n * sizeof(HaloRec); }
// A face buffer of capacity cap: [SlabHdr][cap x SlabRec migrants][cap x HaloRec halo copies], i.e. both messages at their largest.
__host__ __device__ __forceinline__ size_t slab_face_mig_off() { return sizeof(SlabHdr); }
__host__ __device__ __forceinline__ size_t slab_face_halo_off(uint32_t cap) { return slab_mig_msg_bytes(cap); }
__host__ __device__ __forceinline__ size_t slab_face_bytes(uint32_t cap) { return slab_mig_msg_bytes(cap) + slab_halo_msg_bytes(cap); }

// Start of a substep on a slab rank [z0, z1): classify every local slot by its CURRENT position.
//   stale ghost                      -> dead
//   owned, still inside              -> stays; copied to the neighbour as a ghost if in a boundary layer
//   owned, crossed into a neighbour  -> record sent as a migrant; kept here as a ghost if it sits in the
//                                       adjacent layer, otherwise dead
// !COMPACT (sph_slab_pack, caller-owned buffers): every record goes out as a SlabRec, counted in RecLo / RecHi.
// COMPACT (the engine-owned face buffers): sendLo / sendHi point at a face buffer; halo copies and migrants are counted apart
// (HaloLo .. MigHi).
template <bool COMPACT>
__global__ __launch_bounds__(kBlock) void k_slab_pack(SimK k, int z0, int z1, int hasLo, int hasHi, float4* __restrict__ pos,
                                                      const float4* __restrict__ vel, const float2* __restrict__ rp,
                                                      const float* __restrict__ foam, const float4* __restrict__ acc, int nBound, SlabRec* __restrict__ sendLo,
                                                      SlabRec* __restrict__ sendHi, uint32_t capLo, uint32_t capHi,
                                                      uint32_t* __restrict__ counters, const uint32_t* __restrict__ cellStart, int layerCells) {
    const int gzLocal = z1 - z0 + 2;                    // the rank's layers plus one ghost layer each side (k holds the GLOBAL grid here)
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int n = min(nBound, (int)counters[kSlabCntLive]);
    if ((int)(blockIdx.x * kBlock) >= n) return;       // whole block beyond the data
    // cellStart != nullptr: the slots are still in the order of the last counting sort (z-major) and nothing moved a
    // particle by more than kSlabJump cell layers since (unchanged container; a substep that did is reported, slab_check_layer_move).  Everything this pass acts on --
    // stale ghosts, face particles, migrants -- then entered that substep in one of the kSlabDepth lowest or highest
    // local layers, i.e. sits in two slot ranges at the ends; blocks in between have nothing to do.
    bool inEnds = true;
    if (cellStart && gzLocal > 2 * kSlabDepth) {
        const int endLo = (int)cellStart[kSlabDepth * layerCells], startHi = (int)cellStart[(gzLocal - kSlabDepth) * layerCells];
        const int b0 = (int)(blockIdx.x * kBlock);
        if (b0 >= endLo && b0 + kBlock <= startHi) return;
        // exactly the two ranges, slot by slot: the boundary-first substep (sph_slab_step_begin) runs this pass while the SPH
        // pass is still writing the slots in between
        inEnds = i < endLo || i >= startHi;
    }
    bool toLoBuf = false, toHiBuf = false;
    SlabRec r;
    r.px = r.py = r.pz = r.vx = r.vy = r.vz = r.rho = r.prs = r.foam = 0.0f; r.id = 0; r.flags = 0; r.pad = 0;
    r.ax = r.ay = r.az = r.pad2 = 0.0f;
    uint32_t fLo = 0, fHi = 0;
    if (i < n && inEnds) {
        const float4 P = pos[i];
        uint32_t flags = fbits(P.w);
        if (!(flags & F_DEAD)) {
            if (flags & F_HALO) {
                pos[i].w = bitsf(flags | F_DEAD);
            } else {
                const int cz = cell_z_global(k, P.z);
                const bool goLo = cz < z0, goHi = cz >= z1;
                const float4 V = vel[i];
                const float2 RP = rp[i];
                r.px = P.x; r.py = P.y; r.pz = P.z; r.vx = V.x; r.vy = V.y; r.vz = V.z;
                r.rho = RP.x; r.prs = RP.y; r.foam = foam[i]; r.id = fbits(V.w);
                if (acc) { const float4 A = acc[i]; r.ax = A.x; r.ay = A.y; r.az = A.z; }
                toLoBuf = hasLo && (goLo || cz == z0);
                toHiBuf = hasHi && (goHi || cz == z1 - 1);
                fLo = goLo ? flags : (flags | F_HALO);
                fHi = goHi ? flags : (flags | F_HALO);
                if (goLo) pos[i].w = bitsf(cz == z0 - 1 ? (flags | F_HALO) : (flags | F_DEAD));
                if (goHi) pos[i].w = bitsf(cz == z1 ? (flags | F_HALO) : (flags | F_DEAD));
            }
        }
    }
    if (!COMPACT) {
        r.flags = fLo;
        wave_append(sendLo, &counters[kSlabCntRecLo], capLo, toLoBuf, r);
        r.flags = fHi;
        wave_append(sendHi, &counters[kSlabCntRecHi], capHi, toHiBuf, r);
    } else {
        HaloRec hr;
        hr.px = r.px; hr.py = r.py; hr.pz = r.pz; hr.vx = r.vx; hr.vy = r.vy; hr.vz = r.vz; hr.rho = r.rho; hr.prs = r.prs; hr.id = r.id;
        char* const fl = reinterpret_cast<char*>(sendLo);
        char* const fh = reinterpret_cast<char*>(sendHi);
        r.flags = fLo; hr.flags = fLo;
        wave_append(reinterpret_cast<SlabRec*>(fl + slab_face_mig_off()), &counters[kSlabCntMigLo], capLo, toLoBuf && !(fLo & F_HALO), r);
        wave_append(reinterpret_cast<HaloRec*>(fl + slab_face_halo_off(capLo)), &counters[kSlabCntHaloLo], capLo, toLoBuf && (fLo & F_HALO), hr);
        r.flags = fHi; hr.flags = fHi;
        wave_append(reinterpret_cast<SlabRec*>(fh + slab_face_mig_off()), &counters[kSlabCntMigHi], capHi, toHiBuf && !(fHi & F_HALO), r);
        wave_append(reinterpret_cast<HaloRec*>(fh + slab_face_halo_off(capHi)), &counters[kSlabCntHaloHi], capHi, toHiBuf && (fHi & F_HALO), hr);
    }
}

// What a received record tells about the exchange's one assumption -- no particle crosses more than one cell layer in z per
// substep.  An OWNED record (a migrant) must land inside the receiver's layers, and
// not in the layer next to its OTHER face: that layer's particles are halo copies on a third rank, and this exchange is already
// past the point where the receiver could have made one.  Otherwise the run goes on, but no longer equals the single-domain run:
// kSlabFlagLayerJump.  (fromLo: the record came from the lower neighbour.)
struct SlabGeom {
    float gminz, cellSize;
    int gzGlobal, z0, z1, hasLo, hasHi;
};
__device__ __forceinline__ bool slab_record_misplaced(const SlabGeom& g, const SlabRec& r, bool fromLo) {
    if (r.flags & (F_HALO | F_DEAD)) return false;
    const int cz = cell_axis(r.pz, g.gminz, g.cellSize, g.gzGlobal);
    if (cz < g.z0 || cz >= g.z1) return true;                               // belongs to a rank further on
    if (g.z1 - g.z0 < 2) return false;
    return fromLo ? (g.hasHi && cz == g.z1 - 1) : (g.hasLo && cz == g.z0);  // a third rank needed its halo copy in this very exchange
}
// A received migrant (or an uncompacted record) into slot d, and what it tells (above).
__device__ __forceinline__ void slab_store_record(const SlabRec& r, int d, float4* __restrict__ pos, float4* __restrict__ vel, float2* __restrict__ rp,
                                                  float* __restrict__ foam, float4* __restrict__ acc, const SlabGeom& g, bool fromLo, uint32_t* __restrict__ counters) {
    pos[d] = make_float4(r.px, r.py, r.pz, bitsf(r.flags));
    vel[d] = make_float4(r.vx, r.vy, r.vz, bitsf(r.id));
    rp[d] = make_float2(r.rho, r.prs);
    foam[d] = r.foam;
    acc[d] = make_float4(r.ax, r.ay, r.az, 0.0f);
    if (slab_record_misplaced(g, r, fromLo)) atomicOr(&counters[kSlabCntFlags], kSlabFlagLayerJump);
}

// Append received records behind the local slots.
__global__ __launch_bounds__(kBlock) void k_slab_unpack(const SlabRec* __restrict__ recv, int nRecv, float4* __restrict__ pos,
                                                        float4* __restrict__ vel, float2* __restrict__ rp, float* __restrict__ foam,
                                                        float4* __restrict__ acc, int dstBase, SlabGeom g, int fromLo, uint32_t* __restrict__ counters) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nRecv) return;
    slab_store_record(recv[i], dstBase + i, pos, vel, rp, foam, acc, g, fromLo != 0, counters);
}

// ---- exchange without host round trips: the record counts travel in a header in front of the payload ----
constexpr uint32_t kSlabMagic = 0x48414c4fu;            // "HALO": first word of a face's header
// Behind k_slab_pack<true>: the headers of both send faces, the counts of this pack for the host, the running counts back to zero.
// msg: the records this engine's messages of THIS exchange will carry (the host's plan, slab_plan in sph_engine.hip).
__global__ void k_slab_headers2(uint32_t* __restrict__ counters, char* __restrict__ faceLo, char* __restrict__ faceHi, uint32_t cap, SlabMsg msg) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t ex = counters[kSlabCntExchange];
    for (int d = 0; d < 2; ++d) {
        char* f = d ? faceHi : faceLo;
        const uint32_t nh = counters[kSlabCntHaloLo + d], nm = counters[kSlabCntMigLo + d];
        if (nh > cap || nm > cap) atomicOr(&counters[kSlabCntFlags], kSlabFlagSendOverflow);
        if (f) {
            SlabHdr h;
            h.magic = kSlabMagic; h.nHalo = min(nh, cap); h.nHaloTrue = nh; h.nMig = min(nm, cap); h.nMigTrue = nm; h.exchange = ex;
            h.msgHalo = msg.halo[d]; h.msgMig = msg.mig[d];
            for (int i = 0; i < 8; ++i) h.pad[i] = 0u;
            *reinterpret_cast<SlabHdr*>(f) = h;
        }
        counters[kSlabCntLastHaloLo + d] = nh; counters[kSlabCntLastMigLo + d] = nm;
        counters[kSlabCntHaloLo + d] = 0u; counters[kSlabCntMigLo + d] = 0u;
        counters[kSlabCntPackedLo + d] = nh + nm;
    }
    counters[kSlabCntExchange] = ex + 1u;
}
// What of a received face may be used: the header must be one, and the counts are cut to what the MESSAGES carried
// (msgHalo / msgMig records: the receiver sized them from the sender's counts of two exchanges ago; more than that -> kSlabFlagTruncated).
struct FaceCounts { uint32_t nHalo, nMig; bool bad, more, sized; };
__device__ __forceinline__ FaceCounts slab_face_counts(const char* __restrict__ face, uint32_t cap, uint32_t msgHalo, uint32_t msgMig) {
    FaceCounts c{0u, 0u, false, false, false};
    if (!face) return c;
    const SlabHdr h = *reinterpret_cast<const SlabHdr*>(face);
    if (h.magic != kSlabMagic || h.nHalo > cap || h.nMig > cap) { c.bad = true; return c; }
    c.nHalo = min(h.nHalo, msgHalo); c.nMig = min(h.nMig, msgMig);
    c.more = h.nHaloTrue > c.nHalo || h.nMigTrue > c.nMig;
    c.sized = h.msgHalo != msgHalo || h.msgMig != msgMig;      // the sender's messages carried another number of records than this end received
    return c;
}
// Appends the face received from direction d behind slot counters[Live] (+ the records of the face unpacked first, otherFirst: the one
// from direction 1 - d, or nullptr): halo copies, then migrants.  msg: the records this engine's receives were sized for.
__global__ __launch_bounds__(kBlock) void k_slab_unpack2(const char* __restrict__ face, const char* __restrict__ otherFirst, uint32_t cap, SlabMsg msg,
                                                         float4* __restrict__ pos, float4* __restrict__ vel,
                                                         float2* __restrict__ rp, float* __restrict__ foam, float4* __restrict__ acc, uint32_t* __restrict__ counters,
                                                         uint32_t slotCap, SlabGeom g, int d) {
    const FaceCounts c = slab_face_counts(face, cap, msg.halo[d], msg.mig[d]);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.nHalo + c.nMig) return;
    const FaceCounts o = slab_face_counts(otherFirst, cap, msg.halo[1 - d], msg.mig[1 - d]);
    const uint32_t dst = counters[kSlabCntLive] + o.nHalo + o.nMig + i;
    if (dst >= slotCap) { atomicOr(&counters[kSlabCntFlags], kSlabFlagSlotOverflow); return; }
    if (i < c.nHalo) {
        const HaloRec r = reinterpret_cast<const HaloRec*>(face + slab_face_halo_off(cap))[i];
        pos[dst] = make_float4(r.px, r.py, r.pz, bitsf(r.flags));
        vel[dst] = make_float4(r.vx, r.vy, r.vz, bitsf(r.id));
        rp[dst] = make_float2(r.rho, r.prs);
        foam[dst] = 0.0f;
        acc[dst] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        slab_store_record(reinterpret_cast<const SlabRec*>(face + slab_face_mig_off())[i - c.nHalo], (int)dst, pos, vel, rp, foam, acc, g, d == 0, counters);
    }
}
__global__ void k_slab_commit2(uint32_t* __restrict__ counters, const char* __restrict__ recvLo, const char* __restrict__ recvHi, uint32_t cap, uint32_t slotCap,
                               SlabMsg msg) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t add = 0u, err = 0u;
    const FaceCounts a = slab_face_counts(recvLo, cap, msg.halo[0], msg.mig[0]), b = slab_face_counts(recvHi, cap, msg.halo[1], msg.mig[1]);
    if (a.bad || b.bad) err |= kSlabFlagBadHeader;
    if (a.more || b.more) err |= kSlabFlagTruncated;
    if (a.sized || b.sized) err |= kSlabFlagSizeMismatch;
    add = a.nHalo + a.nMig + b.nHalo + b.nMig;
    if (err) atomicOr(&counters[kSlabCntFlags], err);
    counters[kSlabCntLive] = min(counters[kSlabCntLive] + add, slotCap);
}

__global__ void k_set_u32(uint32_t* __restrict__ p, uint32_t v) { *p = v; }

// Owned particles of a slab rank as 64-byte records (pos3, vel3, acc3, rho, P, foam, id, flags, 2 pad),
// compacted; *count receives the number written.
struct SlabOut {
    float px, py, pz, vx, vy, vz, ax, ay, az, rho, prs, foam;
    uint32_t id, flags, pad0, pad1;
};
static_assert(sizeof(SlabOut) == 64, "SlabOut is 64 bytes");
__global__ __launch_bounds__(kBlock) void k_slab_download(const float4* __restrict__ pos, const float4* __restrict__ vel,
                                                          const float2* __restrict__ rp, const float* __restrict__ foam,
                                                          const float4* __restrict__ acc, int n, int accValid, SlabOut* __restrict__ out,
                                                          uint32_t cap, uint32_t* __restrict__ count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool own = false;
    SlabOut o;
    o.px = o.py = o.pz = o.vx = o.vy = o.vz = o.ax = o.ay = o.az = o.rho = o.prs = o.foam = 0.0f; o.id = o.flags = o.pad0 = o.pad1 = 0;
    if (i < n) {
        const float4 P = pos[i];
        const uint32_t flags = fbits(P.w);
        if (!(flags & (F_DEAD | F_HALO))) {
            own = true;
            const float4 V = vel[i];
            const float2 RP = rp[i];
            o.px = P.x; o.py = P.y; o.pz = P.z; o.vx = V.x; o.vy = V.y; o.vz = V.z;
            if (accValid) { const float4 A = acc[i]; o.ax = A.x; o.ay = A.y; o.az = A.z; }
            o.rho = RP.x; o.prs = RP.y; o.foam = foam[i]; o.id = fbits(V.w); o.flags = flags;
        }
    }
    wave_append(out, count, cap, own, o);
}

}  // namespace sph
