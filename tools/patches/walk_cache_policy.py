"""Variant patch: a compile-time cache policy for every class of memory access of k_sph_walk (the shipped kernel uses the default
policy for its loads and non-temporal output stores).  Each switch is the cache-policy operand of a buffer load (gfx950: 1 = sc0, 2 = nt, 16 = sc1; nt and sc1 loads are
served by L2 without allocating in the CU's L1), 0 = the shipped instruction:
  -DSPH_WALK_POLICY_WINDOW=p   (a) the window staging loads of plan()
  -DSPH_WALK_POLICY_OWN=p      (b) the target's own S.P / S.V / S.own loads (through buffer resources when p != 0)
  -DSPH_WALK_POLICY_BOUNDS=p   (c) the 18 cellStart run bounds (through a buffer resource when p != 0)
  -DSPH_WALK_POLICY_GATHER=p   (d) the walks' gathers of sweeps 2 / 3
  -DSPH_WALK_POLICY_STORE=0    (e) the five output stores of store_fields as plain stores (shipped, and the default here: 1 = non-temporal)
The loads of the unstaged rows and of the exact fallback sweeps keep the default policy.  With no switch set the kernel's code is the
shipped one.  (profiles/r29_walk_cache_policy_counters.json was measured before the non-temporal stores shipped: its "parent" is
-DSPH_WALK_POLICY_STORE=0 and its "e" is today's kernel.)  usage: tools/build_variant.sh <name> tools/patches/walk_cache_policy.py -DSPH_WALK_POLICY_WINDOW=16 ..."""
import os, sys
d = sys.argv[1]


def sub(s, old, new, count=1):
    assert s.count(old) == count, (old, s.count(old))
    return s.replace(old, new)


p = os.path.join(d, "sph_walk.h")
s = open(p).read()
s = sub(s, '''typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t byteOff) {
    const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)byteOff, 0, 0);   // out of range reads return 0, never fault
''', '''#ifndef SPH_WALK_POLICY_WINDOW
#define SPH_WALK_POLICY_WINDOW 0
#endif
#ifndef SPH_WALK_POLICY_OWN
#define SPH_WALK_POLICY_OWN 0
#endif
#ifndef SPH_WALK_POLICY_BOUNDS
#define SPH_WALK_POLICY_BOUNDS 0
#endif
#ifndef SPH_WALK_POLICY_GATHER
#define SPH_WALK_POLICY_GATHER 0
#endif
#ifndef SPH_WALK_POLICY_STORE
#define SPH_WALK_POLICY_STORE 1
#endif

typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

template <int POLICY = 0>
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t byteOff) {
    const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)byteOff, 0, POLICY);   // out of range reads return 0, never fault
''')
# (b) the target's own loads: s < n, so the resources over the n records bound them
s = sub(s, '''    const float4 P = S.P(s), V = S.V(s), O = S.own[s];
    if (live && special_slot(k, S, in, out, order, s, P, V, O)) live = false;
    Own o;''', '''    float4 P, V, O;
    if constexpr (SPH_WALK_POLICY_OWN == 0) { P = S.P(s); V = S.V(s); O = S.own[s]; }
    else {
        const __amdgpu_buffer_rsrc_t bufP = __builtin_amdgcn_make_buffer_rsrc((void*)S.pv, 0, (int)((uint32_t)n * 32u), 0x00020000);
        const __amdgpu_buffer_rsrc_t bufO = __builtin_amdgcn_make_buffer_rsrc((void*)S.own, 0, (int)((uint32_t)n * 16u), 0x00020000);
        P = buf_load4<SPH_WALK_POLICY_OWN>(bufP, (uint32_t)s * 32u); V = buf_load4<SPH_WALK_POLICY_OWN>(bufP, (uint32_t)s * 32u + 16u);
        O = buf_load4<SPH_WALK_POLICY_OWN>(bufO, (uint32_t)s * 16u);
    }
    if (live && special_slot(k, S, in, out, order, s, P, V, O)) live = false;
    Own o;''')
# (c) the run bounds: cellStart has numCells + 1 entries, rowBase + xhi + 1 <= numCells
s = sub(s, '''    uint32_t qs[9], qe[9];                                 // all 18 run bounds first (independent loads in flight)
''', '''    uint32_t qs[9], qe[9];                                 // all 18 run bounds first (independent loads in flight)
    const __amdgpu_buffer_rsrc_t bufC = __builtin_amdgcn_make_buffer_rsrc((void*)cellStart, 0, (int)(((uint32_t)k.numCells + 1u) * 4u), 0x00020000);
    auto bound_at = [&](int c) -> uint32_t {
        if constexpr (SPH_WALK_POLICY_BOUNDS == 0) return cellStart[c];
        else return __builtin_amdgcn_raw_buffer_load_b32(bufC, c * 4, 0, SPH_WALK_POLICY_BOUNDS);
    };
''')
s = sub(s, '''        const uint32_t a = cellStart[rowBase + xlo], b = cellStart[rowBase + xhi + 1];
        qs[r] = in ? a : 0u; qe[r] = in ? b : 0u;''', '''        const uint32_t a = bound_at(rowBase + xlo), b = bound_at(rowBase + xhi + 1);
        qs[r] = in ? a : 0u; qe[r] = in ? b : 0u;''')
# (a) the windows
s = sub(s, "pre0 = buf_load4(rw, laneOff32);", "pre0 = buf_load4<SPH_WALK_POLICY_WINDOW>(rw, laneOff32);")
s = sub(s, "pre1 = buf_load4(rw, laneOff32 + 2048u);", "pre1 = buf_load4<SPH_WALK_POLICY_WINDOW>(rw, laneOff32 + 2048u);")
s = sub(s, "pre2 = buf_load4(rw, laneOff32 + 4096u);", "pre2 = buf_load4<SPH_WALK_POLICY_WINDOW>(rw, laneOff32 + 4096u);")
# (d) the gathers
s = sub(s, "J = buf_load4(bufPV, qb); JV = buf_load4(bufPV, qb + 16u);",
        "J = buf_load4<SPH_WALK_POLICY_GATHER>(bufPV, qb); JV = buf_load4<SPH_WALK_POLICY_GATHER>(bufPV, qb + 16u);")
# (e) the stores (store_fields<STREAM> of sph_pass.h)
s = sub(s, "if (live) store_fields<true>(k, out, s,", "if (live) store_fields<(SPH_WALK_POLICY_STORE != 0)>(k, out, s,")
open(p, "w").write(s)

