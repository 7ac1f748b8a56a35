// Counter-based Philox4x32-10 streams of the library (sampler.cpp, dsm.cpp): standard normals by Box-Muller and standardisable gamma
// variates (Marsaglia & Tsang), keyed by (seed, GLOBAL sample index, draw, element) so a stream does not depend on how the batch is
// sharded over GPUs.  Both including units are compiled with -ffp-contract=off (csrc/build.py), so the same key gives the same bits in each.
//
// Draw words in use (the draw word enters the counter as bits 8..31 of c1 and bits 0..39 of c3, see philox_normal4):
//   0, 1, ...            the samplers' step draws (mcvd_sampler_run, mcvd_randn callers)
//   2^32 + k             the k-th conditioning-noise draw of a noise_in_cond forward (model.cpp OP_CONDNOISE)
//   bit 39 set           the gamma stream of any of the above (philox_uniform4)
//   bit 40 set           the denoising score-matching loss's z (dsm.cpp DSM_DRAW; with bit 39 as well under gamma)
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
    const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);    // (0,1)
    const float u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u3 = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, cs0, s1, cs1;
    sincosf(6.283185307179586f * u1, &s0, &cs0);
    sincosf(6.283185307179586f * u3, &s1, &cs1);
    return make_float4(r0 * cs0, r0 * s0, r1 * cs1, r1 * s1);
}

// 4 uniforms in (0,1) for counter (sample, draw, ctr); the gamma sampler's stream (bit 39 of the draw word keeps it apart from
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

// Gamma(shape k, scale 1) by Marsaglia & Tsang (2000): d = k - 1/3, c = 1/sqrt(9 d); x ~ N(0,1), v = (1 + c x)^3, accept when
// v > 0 and log u < x^2/2 + d - d v + d log v.  k < 1 uses Gamma(k + 1) * u^(1/k).  Acceptance > 95 % for k >= 1; after 8 rejections
// the last candidate is kept (probability < 1e-10).  Counter-based: element e, attempt j -> Philox counter 8 e + j.
__device__ inline float philox_gamma(float k, uint64_t seed, uint64_t sample, uint64_t draw, uint64_t elem) {
    const float kk = k < 1.0f ? k + 1.0f : k;
    const float d = kk - (1.0f / 3.0f), c = rsqrtf(9.0f * d);
    float g = d;
    for (int j = 0; j < 8; ++j) {
        const float4 u = philox_uniform4(seed, sample, draw, elem * 8 + (uint64_t)j);
        const float r = sqrtf(-2.0f * logf(u.x));
        const float x = r * cosf(6.283185307179586f * u.y);
        const float t = 1.0f + c * x;
        const float v = t * t * t;
        g = d * fmaxf(v, 1e-30f);
        if (v > 0.0f && logf(u.z) < 0.5f * x * x + d - d * v + d * logf(v)) {
            if (k < 1.0f) g *= powf(u.w, 1.0f / k);
            break;
        }
    }
    return g;
}

}  // namespace mcvd
