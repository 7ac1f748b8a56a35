// What the four Winograd F(2x2, 3x3) kernels (conv_wino.cpp, conv_wino2h.cpp, conv_wino3.cpp, conv_wino3p.cpp) have in common:
// the vector types, SiLU, the bf16 split, the epilogue of one (cout, tile) task -- output transform, bias / residual / scale, the
// store, the GroupNorm partial of the final values -- and the host side's launch chain.
#pragma once

#include <type_traits>

#include "../common.h"

namespace mcvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wino_silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// (lo, hi) -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned wino_cvt_pk_bf16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// exact three-way split of an adjacent register pair into packed bf16 pairs (w1 the leading pieces): the two subtractions of a
// level are one v_pk_add_f32
__device__ __forceinline__ void wino_split3(f32x2 v, unsigned& w1, unsigned& w2, unsigned& w3) {
    w1 = wino_cvt_pk_bf16(v.x, v.y);
    const f32x2 h = {__builtin_bit_cast(float, w1 << 16), __builtin_bit_cast(float, w1 & 0xffff0000u)};
    v = v - h;
    w2 = wino_cvt_pk_bf16(v.x, v.y);
    const f32x2 g = {__builtin_bit_cast(float, w2 << 16), __builtin_bit_cast(float, w2 & 0xffff0000u)};
    v = v - g;
    w3 = wino_cvt_pk_bf16(v.x, v.y);
}

// The epilogue's pieces are MACROS: as __forceinline__ functions they compute the same bits, but every instantiation came out 16 to 31
// instructions longer and the register allocation of the K loops moved (profiles/wino_shared_isa.txt).  They expand inside a kernel
// and name their inputs; what they declare is listed with each.
//
// Output transform A^T M A: the 16 position values of a tile (mm[4 * row + column]) -> its 2x2 output block.  Declares y00, y01, y10, y11.
#define WINO_OUT_TRANSFORM(mm)                                                                                  \
    float t0[4], t1[4];                                 /* A^T M */                                             \
    _Pragma("unroll") for (int l = 0; l < 4; ++l) {                                                             \
        t0[l] = mm[0 * 4 + l] + mm[1 * 4 + l] + mm[2 * 4 + l];                                                  \
        t1[l] = mm[1 * 4 + l] - mm[2 * 4 + l] - mm[3 * 4 + l];                                                  \
    }                                                                                                           \
    const float y00 = t0[0] + t0[1] + t0[2], y01 = t0[1] - t0[2] - t0[3];                                       \
    const float y10 = t1[0] + t1[1] + t1[2], y11 = t1[1] - t1[2] - t1[3];

// GroupNorm partial of the FINAL values (ConvArgs::stats) over the tiles of one cout: the 32 lanes of a half-wave (G8: 16 lanes = one
// DPP row per image), each with the 2x2 block v00 .. v11 of its tile.  Pilot-shifted moments: with p = the group's first value (a
// sample of the distribution, so |mean - p| is a few sigma at most and M2 = q - s^2 / n loses a digit, not the result),
// s = sum (v - p) and q = sum (v - p)^2 merge by plain addition -- two v_add_f32 with a DPP source per level, where the exact
// (mean, M2) pairs of conv_wino.cpp cost eight instructions per level and a quarter of the epilogue.  Declares pil (the pilot: lane 0
// / 32 of the wave; G8: 0 / 16 / 32 / 48), sm and qm: behind the last level the group's writer lane (31 of its 32; G8: every lane of
// the row) holds the group's totals.  Uses `lane`.
#define WINO_MERGE(CTRL, ROWMASK)                                                                               \
    {                                                                                                           \
        sm += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sm), CTRL, ROWMASK, 0xf, false)); \
        qm += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, qm), CTRL, ROWMASK, 0xf, false)); \
    }
#define WINO_GN_PARTIAL(G8, v00, v01, v10, v11)                                                                 \
    float pil;                                                                                                  \
    {                                                                                                           \
        const int pv = __builtin_bit_cast(int, v00);                                                            \
        const int s0 = __builtin_amdgcn_readlane(pv, 0), s2 = __builtin_amdgcn_readlane(pv, 32);                \
        if (G8) {                                                                                               \
            const int s1 = __builtin_amdgcn_readlane(pv, 16), s3 = __builtin_amdgcn_readlane(pv, 48);           \
            pil = __builtin_bit_cast(float, (lane & 32) ? ((lane & 16) ? s3 : s2) : ((lane & 16) ? s1 : s0));   \
        } else {                                                                                                \
            pil = __builtin_bit_cast(float, (lane & 32) ? s2 : s0);                                             \
        }                                                                                                       \
    }                                                                                                           \
    const float d0 = v00 - pil, d1 = v01 - pil, d2 = v10 - pil, d3 = v11 - pil;                                 \
    float sm = (d0 + d1) + (d2 + d3);                                                                           \
    float qm = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);                                                       \
    WINO_MERGE(0xB1, 0xf)                   /* quad_perm [1,0,3,2] */                                           \
    WINO_MERGE(0x4E, 0xf)                   /* quad_perm [2,3,0,1] */                                           \
    WINO_MERGE(0x124, 0xf)                  /* row_ror:4 */                                                     \
    WINO_MERGE(0x128, 0xf)                  /* row_ror:8: every lane of a row of 16 holds the row's totals */   \
    if (!G8) WINO_MERGE(0x142, 0xa)         /* row_bcast:15: lanes 16-31 / 48-63 add the totals of the row below */

// One (cout, tile) task of the epilogue of conv_wino2h.cpp, conv_wino3.cpp and conv_wino3p.cpp: the tile's 16 position values out of
// the LDS planes [position][32 couts][T tiles] (all 16 from SM0, or, SPLIT, positions 12-15 from SM1: the persistent kernel parks
// them in two buffers), output transform, v = (y * INV + BIAS + R) * out_scale, the
// two float2 stores, and the GroupNorm partial of this cout's tiles, written by the group's writer lane (the writer's arithmetic
// stays inside its branch: hoisted, the whole epilogue is scheduled differently).
//   INV: the fp16 kernels' 1 / (weight scale * activation scale); 1.0f (folds away) for the unscaled bf16 pieces
//   R0, R1: the residual's two pixel pairs;  SMP, VALID: the tile's sample and whether it exists (G8: the second image of the last
//   pair may not);  NP, RR: statistics partials per (sample, cout) and this region's index among them
// Uses a (ConvArgs), T, e_col, e_tile, co (= the task's cout), lane, fin, ydst, pix, W, HW.
#define WINO_EPILOGUE_TASK(G8, SPLIT, SM0, SM1, INV, BIAS, R0, R1, SMP, VALID, NP, RR)                          \
    {                                                                                                           \
        const f32x2 r0 = R0, r1 = R1;                                                                           \
        float mm[16];                                                                                           \
        _Pragma("unroll") for (int xi = 0; xi < 16; ++xi)                                                       \
            mm[xi] = (!(SPLIT) || xi < 12) ? (SM0)[(xi * 32 + e_col) * T + e_tile] : (SM1)[((xi - 12) * 32 + e_col) * T + e_tile]; \
        WINO_OUT_TRANSFORM(mm)                                                                                  \
        const float bvv = BIAS;                                                                                 \
        const float osc = fin ? a.out_scale : 1.0f;                                                             \
        const float v00 = (y00 * (INV) + bvv + r0.x) * osc, v01 = (y01 * (INV) + bvv + r0.y) * osc;             \
        const float v10 = (y10 * (INV) + bvv + r1.x) * osc, v11 = (y11 * (INV) + bvv + r1.y) * osc;             \
        if (co < a.Cout && (VALID)) {                                                                           \
            const long o = ((long)(SMP) * a.Cout + co) * HW + pix;                                              \
            *reinterpret_cast<float2*>(ydst + o) = make_float2(v00, v01);                                       \
            *reinterpret_cast<float2*>(ydst + o + W) = make_float2(v10, v11);                                   \
        }                                                                                                       \
        if (a.stats && fin) {                                                                                   \
            WINO_GN_PARTIAL(G8, v00, v01, v10, v11)                                                             \
            const bool writer = G8 ? (e_tile & 15) == 0 : e_tile == 31;                                         \
            if (writer && co < a.Cout && (VALID)) {                                                             \
                constexpr float NPIX = G8 ? 64.0f : 128.0f;                                                     \
                float* q = a.stats + (((long)(SMP) * a.Cout + co) * (NP) + (RR)) * 2;                           \
                q[0] = sm + NPIX * pil;           /* the partial's sum over its pixels */                       \
                q[1] = fmaxf(qm - sm * sm * (1.0f / NPIX), 0.0f);      /* M2 about the partial's own mean */    \
            }                                                                                                   \
        }                                                                                                       \
    }

// ---------------------------------------------------------------------------------------------------------------------------
// Host side.  Every Winograd kernel asks for more dynamic LDS than the default limit: raise it for this instantiation once per
// device (PerDeviceOnce), then launch.
template <void (*KERNEL)(ConvArgs)>
static int wino_launch_kernel(const ConvArgs& k, dim3 grid, int threads, size_t lds, hipStream_t s) {
    static PerDeviceOnce raised;
    if (raised.first_use()) {
        MCVD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        raised.done();
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds, s, k);
    return 0;
}

// The launchers' dispatch to an instantiation: f(COT, PRO, G8) with integral-constant arguments -- cot sub-tiles of 32 couts;
// PRO 0 raw input, 1 affine, 2 affine + SiLU, 3 (SPADE: conv_wino.cpp only) the SPADE maps of a.gb; G8 whole 8 x 8 images.
template <int V>
using wino_ic = std::integral_constant<int, V>;
template <bool SPADE = false, class F>
static int wino_dispatch(const ConvArgs& a, int cot, F f) {
    auto geo = [&](auto COT, auto PRO) { return (a.H == 8 && a.W == 8) ? f(COT, PRO, std::true_type{}) : f(COT, PRO, std::false_type{}); };
    auto pro = [&](auto COT) {
        if constexpr (SPADE)
            if (a.gb) return geo(COT, wino_ic<3>{});
        if (!a.coef && !a.act) return geo(COT, wino_ic<0>{});
        if (!a.act) return geo(COT, wino_ic<1>{});
        return geo(COT, wino_ic<2>{});
    };
    switch (cot) {
        case 1: return pro(wino_ic<1>{});
        case 2: return pro(wino_ic<2>{});
        default: return pro(wino_ic<3>{});
    }
}

}  // namespace mcvd
