"""Variant patch ("Position gradients of the basis sums"): the target's own g row of k_aggregate_basis_posgrad staged
into a column of dynamic LDS, lds[(b * T + t)][thread], as the forward's accumulators are, instead of read in place 8 planes per candidate.
The candidate's row (the other direction of particle targets, the particles' side of query targets) stays in place.  Blocks of
basis_block(K) threads, B * T * block floats of LDS.  Same terms in the same order: same bytes (the GPU tests pass on the variant).
Measured against the shipped kernel in profiles/r34_ab_conv_posgrad_ldsrow.json; not kept.  usage: convgrad_lds_row.py <csrc dir>"""
import os, sys


def patch(path, pairs):
    s = open(path).read()
    for old, new in pairs:
        assert s.count(old) == 1, old
        s = s.replace(old, new)
    open(path, "w").write(s)


patch(os.path.join(sys.argv[1], "sph_convgrad.h"), [
    ('''template <int T>
__device__ __forceinline__ void convgrad_sums(const BasisK& bk, const ConvGeo& geo, float slope, bool ok, const float* __restrict__ grow, int lane, const float xv[T],
                                              float s[4]) {''',
     '''template <int T, bool LDSROW>
__device__ __forceinline__ void convgrad_sums(const BasisK& bk, const ConvGeo& geo, float slope, bool ok, const float* __restrict__ grow, int lane, const float xv[T],
                                              float s[4], uint32_t stride = 0u) {'''),
    ('''convgrad_step(s, cf, grow[(size_t)(basis_plane(geo.b0, K, n) * C + t * G)], xv[t]);''',
     '''convgrad_step(s, cf, LDSROW ? grow[(uint32_t)(basis_plane(geo.b0, K, n) * T + t) * stride] : grow[(size_t)(basis_plane(geo.b0, K, n) * C + t * G)], xv[t]);'''),
    ('''    const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> gshift;
    const bool fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    const size_t BC''',
     '''    extern __shared__ float lds[];
    const uint32_t stride = blockDim.x;
    const size_t i = ((size_t)blockIdx.x * stride + threadIdx.x) >> gshift;
    const bool fluidOnly = (nb.flags & kAggFluidOnly) != 0;
    const size_t BC'''),
    ('''    const float slope = convgrad_slope(bk.R, bk.half);
    float ax = 0.0f''',
     '''    float* __restrict__ col = lds + threadIdx.x;
    if (OWN_G) {
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int c = (int)lane + t * (int)G;
                col[(uint32_t)(b * T + t) * stride] = c < C ? gOwn[(size_t)(b * C + t * (int)G)] : 0.0f;
            }
    }
    const float slope = convgrad_slope(bk.R, bk.half);
    float ax = 0.0f'''),
    ('''convgrad_sums<T>(bk, geo, slope, inRange, OWN_G ? gOwn : g + (size_t)crow * BC + (size_t)lane, (int)lane, xv, s);''',
     '''if (OWN_G) convgrad_sums<T, true>(bk, geo, slope, inRange, col, (int)lane, xv, s, stride);
                    else convgrad_sums<T, false>(bk, geo, slope, inRange, g + (size_t)crow * BC + (size_t)lane, (int)lane, xv, s);'''),
    ('''convgrad_sums<T>(bk, back, slope, inBack,''', '''convgrad_sums<T, false>(bk, back, slope, inBack,'''),
])
patch(os.path.join(sys.argv[1], "sph_engine.hip"), [
    ("""kPosParticles>{}), dim3(blocks_for(n << bk.gshift)), dim3(kBlock), 0,
                               e->stream, k, nb, bk,""",
     """kPosParticles>{}), dim3(blocks_for(n << bk.gshift, basis_block(cfg->size))), dim3(basis_block(cfg->size)),
                               B * (two ? 2 : 1) * (size_t)basis_block(cfg->size) * sizeof(float), e->stream, k, nb, bk,"""),
    ("""kPosPoints>{}), dim3(blocks_for(m << bk.gshift)), dim3(kBlock), 0,
                               e->stream, k, nb, bk,""",
     """kPosPoints>{}), dim3(blocks_for(m << bk.gshift, basis_block(cfg->size))), dim3(basis_block(cfg->size)),
                               B * (two ? 2 : 1) * (size_t)basis_block(cfg->size) * sizeof(float), e->stream, k, nb, bk,"""),
])
