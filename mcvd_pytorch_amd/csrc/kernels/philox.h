// Counter-based Philox4x32-10 streams of the library (sampler.cpp, dsm.cpp): standard normals by Box-Muller and standardisable gamma
// variates (Marsaglia & Tsang), keyed by (seed, GLOBAL sample index, draw, element) so a stream does not depend on how the batch is
// sharded over GPUs.  Both including units are compiled with -ffp-contract=off (csrc/build.py), so the same key gives the same bits in each.
//
// Key = (seed low word, seed high word).  Counter of (sample, draw, ctr), ctr = the float4 index within the row (normals) or
// 8 * element + attempt (gamma):
//   c0 = ctr low word                       c1 = ctr high word ^ (uint32)(draw << 8)      -- bits 0..23 of the draw word
//   c2 = sample low word                    c3 = sample high word ^ (uint32)(draw >> 24)  -- bits 24..55 of the draw word
// The high word of the sample index and bits 24.. of the draw word share c3: (sample + 2^32, draw) and (sample, draw ^ 2^24) are the
// SAME stream.  Global sample indices must therefore stay below 2^32 (and rows below 2^34 elements, so that the high word of ctr is 0);
// under that rule the draw words in use below give pairwise different (c1, c3) (tests/test_rng_cpu.py).
//
// Draw words in use:
//   0, 1, ...            the samplers' step draws (mcvd_sampler_run, mcvd_randn callers)
//   2^32 + k             the k-th conditioning-noise draw of a noise_in_cond forward (model.cpp OP_CONDNOISE)
//   bit 39 set           the gamma stream of any of the above (philox_uniform4)
//   bit 40 set           the denoising score-matching loss's z (dsm.cpp DSM_DRAW; with bit 39 as well under gamma)
//   bit 41 set           the block init noise of a seeded evaluate_video_gen (runner.py INIT_NOISE_DRAW = 2^41, drawn through mcvd_randn)
//
// Uniforms: u = ((float)(c >> 8) + 0.5f) * 2^-24, in (0, 1]: for c >> 8 >= 2^23 the sum is rounded to fp32 (ties to even), and
// c >> 8 = 2^24 - 1 gives u = 1.0 exactly (a Box-Muller radius of 0, a log u of 0); the smallest u is 2^-25.
#pragma once
#include "../common.h"

namespace mcvd {

__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                             uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// 4 standard normals for counter (sample, draw, elem4)
__device__ __forceinline__ float4 philox_normal4(uint64_t seed, uint64_t sample, uint64_t draw, uint64_t elem4) {
    uint32_t c0 = (uint32_t)elem4, c1 = (uint32_t)(elem4 >> 32) ^ (uint32_t)(draw << 8), c2 = (uint32_t)sample,
             c3 = (uint32_t)(sample >> 32) ^ (uint32_t)(draw >> 24);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);    // (0,1], see above
    const float u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u3 = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, cs0, s1, cs1;
    sincosf(6.283185307179586f * u1, &s0, &cs0);
    sincosf(6.283185307179586f * u3, &s1, &cs1);
    return make_float4(r0 * cs0, r0 * s0, r1 * cs1, r1 * s1);
}

// 4 uniforms in (0,1] for counter (sample, draw, ctr); the gamma sampler's stream (bit 39 of the draw word keeps it apart from
// the normal stream of the same draw index)
__device__ __forceinline__ float4 philox_uniform4(uint64_t seed, uint64_t sample, uint64_t draw, uint64_t ctr) {
    draw |= (1ull << 39);
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32) ^ (uint32_t)(draw << 8), c2 = (uint32_t)sample,
             c3 = (uint32_t)(sample >> 32) ^ (uint32_t)(draw >> 24);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float sc = 1.0f / 16777216.0f;
    return make_float4(((float)(c0 >> 8) + 0.5f) * sc, ((float)(c1 >> 8) + 0.5f) * sc, ((float)(c2 >> 8) + 0.5f) * sc,
                       ((float)(c3 >> 8) + 0.5f) * sc);
}

// Gamma(shape k, scale 1) by Marsaglia & Tsang (2000), the library's one gamma generator: d = k - 1/3, c = 1/sqrt(9 d); x ~ N(0,1),
// v = (1 + c x)^3, accept when v > 0 and log u < x^2/2 + d - d v + d log v; the variate is d v.  k < 1 draws at k + 1 and multiplies the
// accepted variate by u.w^(1/k).  Acceptance > 95 % for k >= 1; after 8 rejections the last candidate d max(v, 1e-300) is kept as it is
// (probability < 1e-10).  Counter-based: element e, attempt j -> Philox counter 8 e + j; of its four uniforms x comes from (u.x, u.y) by
// Box-Muller's cosine branch, u.z decides and u.w is the k < 1 factor.
// The candidate and its acceptance test are evaluated in fp64 from the fp32 uniforms.  The samplers and the loss draw at k = k_cum[label],
// which reaches ~2.5e10 at label 0: an fp32 test evaluates d - d v with ulp(d v) ~ 2e3 against a quantity of order 1, accepts nearly at
// random and distorts the distribution (variance of the standardised draw 11 % high at label 0 and 6 % low at label 250 in a CPU
// emulation of the fp32 test; the loss's pooled variance was 2 % low at B = 64, labels 0..999, measured on the device).
// In fp64 the same cancellation leaves ~1e-5.  The caller rounds theta * g to fp32 once.
__device__ inline double philox_gamma64(float k, uint64_t seed, uint64_t sample, uint64_t draw, uint64_t elem) {
    const double kk = k < 1.0f ? (double)k + 1.0 : (double)k;
    const double d = kk - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;
    for (int j = 0; j < 8; ++j) {
        const float4 u = philox_uniform4(seed, sample, draw, elem * 8 + (uint64_t)j);
        const double x = sqrt(-2.0 * log((double)u.x)) * cos(6.283185307179586 * (double)u.y);
        const double t = 1.0 + c * x;
        const double v = t * t * t;
        g = d * fmax(v, 1e-300);
        if (v > 0.0 && log((double)u.z) < 0.5 * x * x + d - d * v + d * log(v)) {
            if (k < 1.0f) g *= pow((double)u.w, 1.0 / (double)k);
            break;
        }
    }
    return g;
}

}  // namespace mcvd
