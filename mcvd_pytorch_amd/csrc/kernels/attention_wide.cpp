// Self-attention for WIDE heads (head dim D = 160 ... 1024 in steps of 32: n_head_channels = -1 on a wide level, layerspp.py:221-228) on the
// 16-bit matrix pipes, with the split-operand arithmetic of attention_h2.cpp (pieces.h: NP = 3 three bf16 pieces, fp32-equivalent, lazy base-2
// softmax with the score scale riding on Q; NP = 2 two fp16 pieces under the option f16x2, operands times 2^4, probabilities times 2^12).
//
// Beyond D = 128 the Q pieces and the O accumulators of a whole head do not fit a lane (D = 768, NP = 3: 288 + 384 registers), so the HEAD DIM
// is divided: one workgroup = AW_NW waves = ONE tile of 32 queries, and wave w owns a contiguous slice of the D / 32 channel tiles
//     n_w = DT / NW + (w < DT % NW),   first tile f_w = w (DT / NW) + min(w, DT % NW)        (uneven: D = 160 has five tiles)
// -- the Q pieces and the O accumulators of those channels only (at most TW = ceil(DT / NW) <= 4 tiles: the register profile of
// attn_h2_kernel<NP, 4>).  Per key tile of 32:
//   1. every wave with channels computes the PARTIAL S^T (32 keys x 32 queries, 16 registers) over its slice.  Its K operands come straight
//      from global memory in the MFMA A-operand order, by the very index expression that loads Q (lane = key, half h, element e of step st
//      <-> channel 16 st + 2e + h), and are split in the lane that feeds them to the matrix pipe: each K element is fetched and split ONCE
//      per workgroup, no K tile is staged in the LDS and nothing is shared between waves;
//   2. the partials go through the LDS -- image [buffer t & 1][wave][quad q][64 lanes][4 dwords], register r = 4q + dword, one
//      ds_write_b128 / ds_read_b128 per quad, slots of different waves disjoint -- and behind ONE workgroup barrier every wave adds them
//      IN WAVE ORDER 0 ... NWA - 1 (NWA = min(NW, DT) waves have channels): a fixed order and no atomics, so the result is bit-identical from
//      run to run and does not depend on B, on the grid or on how a batch is split into calls.  Two buffers: a wave that writes tile t + 1
//      has passed barrier t, which every wave reaches only after it has read tile t - 1;
//   3. every wave with channels runs the same in-lane softmax on the same sum (redundantly: identical bits in every wave);
//   4. ... and the PV product for ITS output channels: V operands straight from global memory too (lane = channel, half h, step s2: the
//      two float4 at keys 16 s2 + 8 g + 4 h, g = 0, 1, are dwords (2g, 2g + 1) of the operand -- the keys whose probabilities sit in
//      accumulator registers 8 s2 + 4g ... + 3 of the S^T tile, attention_h2.cpp's PV convention), split in the lane.
// A wave without channels (w >= DT, D = 160 ... 224) takes part in the barriers and in nothing else.
// Block id -> (sample-head, query tile) as attention_h2.cpp: the query tiles of one (sample, head) run on ONE XCD, adjacent in time.
// Serves D % 32 == 0, 160 <= D <= 1024, HW % 32 == 0, any number of heads.  LDS: 2 x NWA x 4 KB <= 64 KB.
// Measured against the one-thread-per-query kernel, which is what ran above D = 256 before: x 325 ... 1700; against the fp32 flash kernel
// on 160 ... 256: see attn_kernels.h (profiles/attn_wide_time.txt).  What it leaves on the table, by instruction count and not by a counter
// pass: of the ~600 vector instructions a wave issues per key tile at TW = 1 about half -- the sum of the partials, the softmax and the
// split of P -- are repeated by every wave of the workgroup; 32 queries per workgroup stream K and V four times as often as
// attention_h2.cpp's 128.
#include <math.h>

#include "../common.h"
#include "pieces.h"

namespace mcvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int AW_NW = 8;                              // waves per workgroup
constexpr int AW_D_MIN = 160, AW_D_MAX = 1024;        // head dims served
constexpr int AW_XCH = 1024;                          // dwords of one wave's S^T partial in the exchange image: 4 quads x 64 lanes x 4
constexpr float AW_P_LOG = 8.317766166719343f;        // 12 ln 2: NP = 2 probabilities times 2^12 (attention_h2.cpp AH_P_LOG)
constexpr float AW_LOG2E = 1.4426950408889634f;
constexpr float AW_LAZY = 40.0f;                      // NP = 3: the exponent reference moves only when a tile maximum outgrows it by 2^40 (AH_LAZY)

// TW = 1 (D <= 256) asks for four waves per SIMD = TWO workgroups per CU: NP = 3 then spills 15 registers (142 -> 128) and is still the faster
// build, D = 256 at 32 x 32: 0.74 against 0.86 ms, at 16 x 16 0.060 against 0.068 ms (A/B of the two builds in one session, profiles/attn_wide_time.txt)
template <int NP, int TW>   // TW = channel tiles per wave at most = ceil(D / 32 / AW_NW)
__global__ __launch_bounds__(64 * AW_NW, TW == 1 ? 4 : 2) void attn_wide_kernel(const float* __restrict__ qkv, float* __restrict__ out, int C, int heads, int S, int DT,
                                                                float scale_s, int nbh, int nqt) {
    typedef Pieces<NP> PX;
    constexpr float OPS = NP == 2 ? PX::ACT_SCALE : 1.0f;          // operand scale of Q, K, V
    extern __shared__ __attribute__((aligned(16))) float smem_attn_wide[];
    u32x4* sX = reinterpret_cast<u32x4*>(smem_attn_wide);          // [2 buffers][NWA waves][4 quads][64 lanes] of 4 dwords

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bh = (slot / nqt) * 8 + xcd, qt = slot - (slot / nqt) * nqt;
    if (bh >= nbh) return;                          // (the whole workgroup)
    const int b = bh / heads, hd = bh - b * heads;
    const int D = 32 * DT;
    const int nwa = min(AW_NW, DT);                 // waves with channels
    const int tb = DT / AW_NW, tr = DT - tb * AW_NW;
    const int nt = tb + (wave < tr ? 1 : 0);        // this wave's channel tiles ...
    const int ft = wave * tb + min(wave, tr);       // ... from tile ft on
    const int ntiles = S / 32;
    if (nt == 0) {                                  // no channels: the barriers of the key loop and nothing else
        for (int t = 0; t < ntiles; ++t) __syncthreads();
        return;
    }
    const float* qb = qkv + ((long)b * 3 * C + hd * D + ft * 32) * S;      // the wave's first channel of q, k, v
    const float* kb = qb + (long)C * S;
    const float* vb = kb + (long)C * S;
    const int q0 = qt * 32;

    // Q pieces of the wave's channels: lane (query l31, half) holds channels 16 st + 2e + half, e = 0..7 of every step; dword j = elements (2j, 2j+1)
    const float qs = NP == 3 ? scale_s * AW_LOG2E : OPS;          // NP = 3: the score scale and log2(e) ride on Q
    u32x4 qp[2 * TW][NP];
#pragma unroll
    for (int st = 0; st < 2 * TW; ++st)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool have = (st >> 1) < nt;
            const float* qc = qb + (long)(16 * st + 4 * j) * S + q0;      // row c0 = 16 st + 4 j + half (and c0 + 2), query l31: as K
            const float a0 = have ? qc[half * S + l31] : 0.0f;
            const float a1 = have ? qc[half * S + l31 + 2 * S] : 0.0f;
            unsigned w[NP];
            PX::template split<false>(a0 * qs, a1 * qs, w);
#pragma unroll
            for (int p = 0; p < NP; ++p) qp[st][p][j] = w[p];
        }

    f32x16 o[TW];
#pragma unroll
    for (int ct = 0; ct < TW; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[ct][r] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f;

    // The raw operands of a key tile are 16 + 16 registers per channel tile.  Up to two tiles per wave (D <= 512) they are PREFETCHED: K of
    // key tile t + 1 is requested behind the S product of tile t and lands under its exchange, softmax and PV product; V of tile t is
    // requested in front of the S product.  Beyond, Q pieces and O accumulators leave no room: loaded where they are consumed.
    constexpr bool PF = TW <= 2;
    // addresses = a wave-uniform row pointer + ONE per-lane offset per operand.  With the lane folded into every row address the compiler
    // kept the 16 + 4 row addresses per channel tile in vector register pairs across the key loop: NP = 3 took 172 registers at TW = 1 and
    // spilled 27 / 40 / 112 at TW = 2 / 3 / 4; written this way 128 (TW = 1, by its launch bounds) / 222 / 212 / 252, no spill from TW = 2 on
    const unsigned klane = half * S + l31, klane2 = klane + 2 * S;      // K: row c0 = 16 s + 4 j + half (and c0 + 2), key l31
    const unsigned vlane = l31 * S + 4 * half;                          // V: row l31 of the tile, keys 4 half ... + 3 of the float4
    float kr[PF ? 2 * TW : 1][8];                     // step s: channels (c0, c0 + 2) of dword j at [2j], [2j + 1]
    f32x4 vr[PF ? TW : 1][4];                         // tile ct: the float4 of (s2, g) at [2 s2 + g]
    auto kload = [&](int t) {
        const float* kt = kb + t * 32;              // (wave-uniform; the lane's part of the address is klane)
#pragma unroll
        for (int s = 0; s < 2 * TW; ++s)
            if ((s >> 1) < nt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* kc = kt + (long)(16 * s + 4 * j) * S;
                    kr[PF ? s : 0][2 * j] = kc[klane];
                    kr[PF ? s : 0][2 * j + 1] = kc[klane2];
                }
            }
    };
    auto vload = [&](int t) {
        const float* vt = vb + t * 32;              // (wave-uniform; the lane's part is vlane)
#pragma unroll
        for (int ct = 0; ct < TW; ++ct)
            if (ct < nt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) vr[PF ? ct : 0][i] = *reinterpret_cast<const f32x4*>(vt + (long)ct * 32 * S + 16 * (i >> 1) + 8 * (i & 1) + vlane);
            }
    };
    if constexpr (PF) kload(0);

    for (int t = 0; t < ntiles; ++t) {
        if constexpr (PF) vload(t);
        // ---- partial S^T over the wave's channels: A = K pieces (lane = key l31), B = Q pieces (NP = 2: times 2^8)
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const float* kt = kb + t * 32;
#pragma unroll
        for (int s = 0; s < 2 * TW; ++s) {
            if ((s >> 1) < nt) {                      // (wave-uniform)
                u32x4 kp[NP];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* kc = kt + (long)(16 * s + 4 * j) * S;
                    const float a0 = PF ? kr[PF ? s : 0][2 * j] : kc[klane];
                    const float a1 = PF ? kr[PF ? s : 0][2 * j + 1] : kc[klane2];
                    unsigned w[NP];
                    PX::template split<false>(a0 * OPS, a1 * OPS, w);
#pragma unroll
                    for (int p = 0; p < NP; ++p) kp[p][j] = w[p];
                }
#pragma unroll
                for (int k = 0; k < PX::NPROD; ++k) st = PX::mfma(kp[PX::PA(k)], qp[s][PX::PB(k)], st);
            }
        }
        if constexpr (PF)
            if (t + 1 < ntiles) kload(t + 1);

        // ---- the partials of all waves, added in wave order
        u32x4* xb = sX + (t & 1) * nwa * 256;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            xb[(wave * 4 + q) * 64 + lane] = __builtin_bit_cast(u32x4, f32x4{st[4 * q], st[4 * q + 1], st[4 * q + 2], st[4 * q + 3]});
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 a = __builtin_bit_cast(f32x4, xb[q * 64 + lane]);
            for (int w = 1; w < nwa; ++w) a += __builtin_bit_cast(f32x4, xb[(w * 4 + q) * 64 + lane]);
#pragma unroll
            for (int e = 0; e < 4; ++e) st[4 * q + e] = a[e];
        }

        // ---- online softmax over keys (this lane: 16 keys of query l31; partner lane^32 holds the other 16), as attention_h2.cpp
        float mt = -1e30f;
        if constexpr (NP == 3) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[r]);
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const bool need = mt > m_run + AW_LAZY;
            if (__builtin_amdgcn_ballot_w64(need)) {
                const float m_new = need ? mt : m_run;
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                l_run *= alpha;
#pragma unroll
                for (int ct = 0; ct < TW; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
                m_run = m_new;
            }
            float ps = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - m_run); ps += st[r]; }
            l_run += ps;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] *= scale_s; mt = fmaxf(mt, st[r]); }
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __expf(m_run - m_new);
            const float shift = AW_P_LOG - m_new;
            float ps = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = __expf(st[r] + shift); ps += st[r]; }
            l_run = l_run * alpha + ps;               // per-half partial sum; halves are added at the end
            m_run = m_new;
#pragma unroll
            for (int ct = 0; ct < TW; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
        }
        u32x4 pp[2][NP];                          // B operand of the PV product: step s2, dword j = registers 8 s2 + 2j, + 1
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned w[NP];
                PX::template split<false>(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1], w);
#pragma unroll
                for (int p = 0; p < NP; ++p) pp[s2][p][j] = w[p];
            }

        // ---- O += V * P for the wave's channels: A = V pieces (lane = channel l31 of the tile)
        const float* vt = vb + t * 32;
#pragma unroll
        for (int ct = 0; ct < TW; ++ct) {
            if (ct < nt) {                            // (wave-uniform)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    u32x4 vp[NP];
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const f32x4 v = PF ? vr[PF ? ct : 0][2 * s2 + g] : *reinterpret_cast<const f32x4*>(vt + (long)ct * 32 * S + 16 * s2 + 8 * g + vlane);
                        unsigned wa[NP], wb[NP];
                        PX::template split<false>(v[0] * OPS, v[1] * OPS, wa);
                        PX::template split<false>(v[2] * OPS, v[3] * OPS, wb);
#pragma unroll
                        for (int p = 0; p < NP; ++p) { vp[p][2 * g] = wa[p]; vp[p][2 * g + 1] = wb[p]; }
                    }
#pragma unroll
                    for (int k = 0; k < PX::NPROD; ++k) o[ct] = PX::mfma(vp[PX::PA(k)], pp[s2][PX::PB(k)], o[ct]);
                }
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = (1.0f / OPS) / l_tot;      // NP = 2: l carries the 2^12 of the probabilities, O the 2^12 * 2^4 of P and V
    float* ob = out + ((long)b * C + hd * D + ft * 32) * S + q0 + l31;
#pragma unroll
    for (int ct = 0; ct < TW; ++ct)
        if (ct < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                ob[(long)c * S] = o[ct][r] * inv;
            }
        }
}

bool attention_wide_supported(int C, int heads, int HW) {
    if (heads <= 0 || C % heads != 0) return false;
    const int D = C / heads;
    return D % 32 == 0 && D >= AW_D_MIN && D <= AW_D_MAX && HW > 0 && HW % 32 == 0;
}

template <int NP>
static int attn_wide_launch(const float* qkv, float* out, int B, int C, int heads, int HW, hipStream_t s) {
    const int D = C / heads, DT = D / 32;
    const float scale = (float)pow((double)D, -0.5);   // int(C)**-0.5 as a Python double, then fp32 (layerspp.py:239)
    const float ops = NP == 2 ? Pieces<2>::ACT_SCALE : 1.0f;
    const float scale_s = scale * (1.0f / (ops * ops));      // exact: the S product carries the square of the operand scale
    const int nqt = HW / 32, nbh = B * heads;
    dim3 grid((unsigned)(((nbh + 7) / 8) * 8 * nqt));
    const size_t lds = (size_t)2 * (DT < AW_NW ? DT : AW_NW) * AW_XCH * sizeof(unsigned);
#define AW_CASE(TW)                                                                                                       \
    case TW: {                                                                                                            \
        static PerDeviceOnce raised;                                                                                      \
        if (lds > 48 * 1024 && raised.first_use()) {                                                                      \
            MCVD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_wide_kernel<NP, TW>),                  \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));                   \
            raised.done();                                                                                                \
        }                                                                                                                 \
        hipLaunchKernelGGL((attn_wide_kernel<NP, TW>), grid, dim3(64 * AW_NW), lds, s, qkv, out, C, heads, HW, DT, scale_s, nbh, nqt); \
        break;                                                                                                            \
    }
    switch ((DT + AW_NW - 1) / AW_NW) {
        AW_CASE(1) AW_CASE(2) AW_CASE(3) AW_CASE(4)
    }
#undef AW_CASE
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_attention_wide(const float* qkv, float* out, int B, int C, int heads, int HW, hipStream_t s, int np) {
    MCVD_REQUIRE(attention_wide_supported(C, heads, HW) && (np == 2 || np == 3), "wide-head attention: unsupported (C=%d heads=%d HW=%d np=%d)", C,
                 heads, HW, np);
    return np == 2 ? attn_wide_launch<2>(qkv, out, B, C, heads, HW, s) : attn_wide_launch<3>(qkv, out, B, C, heads, HW, s);
}

}  // namespace mcvd
