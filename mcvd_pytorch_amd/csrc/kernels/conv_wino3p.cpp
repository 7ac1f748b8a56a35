// PERSISTENT form of the three-piece bf16 Winograd convolution (conv_wino3.cpp: same decomposition, same arithmetic, same packed
// weights, bit-identical results): one workgroup per CU walks a contiguous range of (region, cout tile[, K half]) items and the
// staging pipeline of its K loop never drains between them.
//
// Why (profiles/r03_timeline_wino3_conv1x1_b3.txt, r03_wino3_prologue.txt): a workgroup of conv_wino3_kernel spends 9-10 k cycles in
// its prologue (index arithmetic, first memory latency, activation of two patches by all eight waves at once, first transform) and
// 6-7 k in its epilogue before it retires, and the next workgroup of the CU starts ~1.1 us (1.9 k cycles) later: 17-19 k cycles per
// item against 6-12 chunks of 4.7-4.9 k -- 25-35 % of the CU's time without a single MFMA, and with 256-VGPR waves no second
// workgroup can run beside it.  Here
//   * the items of a workgroup are consecutive: [w n / G, (w + 1) n / G) of n = B * regions * cout tiles * K halves, ordered sample,
//     region, cout tile, K half -- the cout tiles of a region follow each other on the same CU (the patch stays in that XCD's L2)
//     and all workgroups walk the cout tiles in step (the weight slice of the moment is shared by the whole chip);
//   * inside a RUN of items of one sample the K loop is one stream of chunks: while the MFMAs of the last chunks of item j run, the
//     staging phases already fetch, activate and transform the first chunks of item j + 1 (its patch offsets come from a per-thread
//     LDS table written during item j, its weights are requested behind the last MFMAs of item j), so an item costs its chunks plus
//     the epilogue and nothing else; the epilogue (all eight waves: accumulators -> LDS -> inverse transform -> global) uses the V
//     buffer the last chunk has just vacated, 16 output channels per round;
//   * a new sample (new GroupNorm coefficient table) ends the run: the pipeline drains and the prologue runs again.  At the batch
//     sizes of BASELINE.json the item ranges are aligned with the samples and every workgroup has exactly one run.
// Shape ids 16 / 17 (17: 2-way K split, the halves are items).  8x8 images stay with conv_wino3_kernel<.., G8> (one item per CU:
// nothing to stream).  The stage of one chunk is the one-shot kernel's, literally: conv_wino3_stage.h holds the constants, the
// named-register map and the macros that load, park, transform and multiply a chunk, with their hand-counted VMEM
// (tools/check_wino_isa.py checks this file too).  This file keeps the slot table, the item stream and its chunk scalars, the
// coefficient table over all of Cin (WP_READ_C) and the epilogue's two-buffer parking; the epilogue's task itself is wino_common.h.
#include <stdlib.h>

#include "../common.h"
#include "conv_wino3_stage.h"

namespace mcvd {

constexpr int WP_NPL = 3;                         // patch-load instructions per thread and chunk (two four-pixel slots + one halo slot)
constexpr int WP_MINCH = 4;                       // chunks per item the stream needs (its staging looks three chunks ahead)

#define W3_SLOT_OFF(word) ((word) & ~3u)          // a word of the slot table: byte offset | bit 0 "zero padding here"
#define W3_TS(i)                                  // no per-phase clock stamps in this kernel

// PRO: 0 raw input, 1 affine, 2 affine + SiLU
template <int COT, int PRO>
__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(86))) void conv_wino3p_kernel(ConvArgs a) {
    // amdgpu_num_vgpr(86): the compiler may allocate v0-v171 (LLVM doubles the number on gfx90a+; conv_wino3.cpp); v172-v255 hold the
    // in-flight loads and the MFMA A operands and are named in the asm text only.
    constexpr int NT = W3_NT, CK = W3_CK, T = W3_T, BCO = 32 * COT, PP = W3_PP, VW = W3_VW, PW = W3_PW;
    constexpr int PSZ = CK * 10 * PP;           // activated input patch of one chunk: [pair 8][10 rows][PP][2 channels]
    constexpr int PBUF = 4096;                  // + dump space for unused patch slots, rounded up to 16 KiB: the epilogue parks four position planes there
    static_assert(PBUF >= PSZ + 8 && PBUF >= 4 * 32 * W3_T, "patch buffer: patch + dump space, and 4 positions x 32 couts x 32 tiles of the epilogue");
    constexpr int NPL = WP_NPL, NPV = 9;
    constexpr bool G8 = false;                  // 8 x 8 images and the timing ablations are the one-shot kernel's: those branches of the
    constexpr int EXP = 0;                      // shared stage vanish here
    constexpr int NQ = 3 * COT;                 // weight quads per position: COT cout sub-tiles x 3 pieces
    constexpr int NA = 2 * NQ;                  // weight loads per wave and chunk
    constexpr int VM_A = NQ + NPL;
    constexpr int PQ = 5;                       // weight quads whose registers hold the first two patches in the prologue
    constexpr long WSTR = 16L * NQ * 256;       // dwords of one chunk of a cout tile's packed weights
    static_assert(NA <= 18 && NA > PQ, "named-register map of conv_wino3_stage.h: v172-v180 patch, v184-v255 eighteen weight quads");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned* sV = reinterpret_cast<unsigned*>(smem);           // [2][VW]
    float* sP = smem + 2 * VW;                  // [2][PBUF]
    float* sCo = sP + 2 * PBUF;                 // [Cin][2] prologue coefficients (A_c, B_c) of the run's sample (PRO only)
    unsigned* sOff = reinterpret_cast<unsigned*>(sCo + 2 * a.Cin);      // [2 item parities][NPL][NT]: byte offset of the slot's (clamped) first pixel from
                                                                        // the chunk's first channel plane | bit 0: the slot is zero padding in this region / unused
                                                                        // (written and read by the owning thread only)
    {   // the kernel descriptor must allocate all 256 registers: the asm statements below name v172-v255 in their text only
        float top;
        asm volatile("" : "={v255}"(top));
    }
    asm volatile("" :: "s"(a.x0), "s"(a.x1), "s"(a.coef), "s"(a.wpb), "s"(a.B), "s"(a.H), "s"(a.W), "s"(a.Cin), "s"(a.CinP), "s"(a.C0),
                 "s"(a.C1), "s"(a.CoutP), "s"(a.ksplit), "s"(a.dbg), "s"(a.wdma));
    const unsigned long long t_start = a.dbg ? __builtin_amdgcn_s_memtime() : 0ull;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int H = a.H, W = a.W, HW = H * W, Cin = a.Cin;
    const int rx_n = W >> 4, rpi = rx_n * (H >> 3);              // regions per image
    const int nct = a.CoutP / BCO;
    const int ksp = a.ksplit >= 2 ? a.ksplit : 1;                // K parts per (region, cout tile): 1, 2, 4 or 8
    const int nch = (a.CinP / CK) / ksp;                         // chunks per item
    const int ips = rpi * nct * ksp;                             // items per sample
    const int n_items = a.B * ips;
    const int it0 = (int)((long)blockIdx.x * n_items / gridDim.x), it1 = (int)((long)(blockIdx.x + 1) * n_items / gridDim.x);
    if (it0 >= it1) return;
    const int rg = __builtin_amdgcn_readfirstlane(wave >> 2);   // rows 2rg, 2rg+1 of B^T d; phase order of the wave
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
#ifdef MCVD_DIAG
    // diagnostics build only (env MCVD_W3P_STAGGER = cycles / 256): the odd workgroups start late.  All workgroups of this kernel run in
    // lock step (same work, same start); the experiment measures what the simultaneous epilogues / weight requests of 256 CUs cost.
    if ((a.wdma >> 8) != 0 && (blockIdx.x & 1)) {
        const unsigned long long until = __builtin_amdgcn_s_memtime() + ((unsigned long long)(a.wdma >> 8) << 8);
        while (__builtin_amdgcn_s_memtime() < until) __builtin_amdgcn_s_sleep(8);
    }
#endif

    // ---- transform role (conv_wino3.cpp): (channel pair, tile) = tid & 255
    const int s_tile = tid & 31, s_cp = (tid & 255) >> 5;
    const int s_ty = s_tile >> 3, s_tx = s_tile & 7;
    const int p_rd = ((s_cp * 10 + 2 * s_ty + rg) * PP + 2 * s_tx) * 2;
    const int v_wr = ((8 * rg * 2 + (s_cp & 1)) * 4 + (s_cp >> 1)) * T + s_tile;

    // ---- patch-load slots, the item-invariant part: p_pk = LDS float index of the slot's first element | channel in chunk << 12
    // (CK for an unused slot: parked in the dump space, never valid)
    unsigned p_pk[NPL];
#pragma unroll
    for (int sl = 0; sl < NPL; ++sl) {
        p_pk[sl] = (unsigned)PSZ | ((unsigned)CK << 12);
        if (sl < 2) {
            const int e = sl * NT + tid;
            if (e < CK * 40) {
                const int ci = e / 40, rem = e - ci * 40, r = rem >> 2, c = (rem & 3) * 4;
                const int cp = (ci >> 2) * 2 + (ci & 1), ce = (ci >> 1) & 1;
                p_pk[sl] = (unsigned)(((cp * 10 + r) * PP + c + 1) * 2 + ce) | ((unsigned)ci << 12);
            }
        } else if (tid < CK * 20) {
            const int e = tid, ci = e / 20, rem = e - ci * 20, r = rem >> 1, c = (rem & 1) * 17;
            const int cp = (ci >> 2) * 2 + (ci & 1), ce = (ci >> 1) & 1;
            p_pk[sl] = (unsigned)(((cp * 10 + r) * PP + c) * 2 + ce) | ((unsigned)ci << 12);
        }
    }
    // the item-dependent part: byte offsets of the slots for a region at (oy0, ox0) -> sOff[tab], bit 0 = "zero padding here"
#define WP_SLOT_TABLE(tab, oy0, ox0, OUT)                                                                       \
    {                                                                                                           \
        int tid_s;       /* an opaque copy of tid: the slot geometry is recomputed per item, not kept live across the K loops */ \
        asm volatile("v_mov_b32 %0, %1" : "=v"(tid_s) : "v"(tid));                                              \
        _Pragma("unroll") for (int sl = 0; sl < NPL; ++sl) {                                                    \
            unsigned off = 1u;                                                                                  \
            if (sl < 2) {                                                                                       \
                const int e = sl * NT + tid_s;                                                                  \
                if (e < CK * 40) {                                                                              \
                    const int ci = e / 40, rem = e - ci * 40, r = rem >> 2, c = (rem & 3) * 4;                  \
                    const int y = (oy0) - 1 + r;                                                                \
                    const bool inside = y >= 0 && y < H;                                                        \
                    off = (unsigned)(ci * HW + min(max(y, 0), H - 1) * W + (ox0) + c) * 4u + (inside ? 0u : 1u); \
                }                                                                                               \
            } else if (tid_s < CK * 20) {                                                                       \
                const int e = tid_s, ci = e / 20, rem = e - ci * 20, r = rem >> 1, c = (rem & 1) * 17;          \
                const int y = (oy0) - 1 + r, x = (ox0) - 1 + c;                                                 \
                const bool inside = y >= 0 && y < H && x >= 0 && x < W;                                         \
                off = (unsigned)(ci * HW + min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)) * 4u + (inside ? 0u : 1u); \
            }                                                                                                   \
            sOff[((tab) * NPL + sl) * NT + tid] = off;                                                          \
            OUT[sl] = off;                                                                                      \
        }                                                                                                       \
    }

    const unsigned wr_voff = (unsigned)lane * 16u;

    // the chunk's stage -- the named registers v172-v255 and the W3_ macros that load, park, transform and multiply -- is conv_wino3_stage.h
#define WP_READ_C(ch, cfv)                                                                                      \
    {                                                                                                           \
        _Pragma("unroll") for (int sl = 0; sl < NPL; ++sl) {                                                    \
            cfv[sl] = f32x2{1.0f, 0.0f};                                                                        \
            if (PRO >= 1) {                                                                                     \
                const int cch = min((ch) * CK + (int)((p_pk[sl] >> 12) & (CK - 1)), Cin - 1);                   \
                cfv[sl] = *reinterpret_cast<const f32x2*>(sCo + cch * 2);                                       \
            }                                                                                                   \
        }                                                                                                       \
    }
    /* staging of the stream at chunk g (V(g) is being multiplied): park chunk g+2 (absolute chunk CH2, patch buffer par: g+2 and g
       have the same parity) -- its raw values were requested one chunk ago together with the flags pfl --, request chunk g+3
       (absolute chunk CH3, slot table TAB3), transform chunk g+1 (buffers par ^ 1) */
#define WP_VALU_PHASE(par, CH2, CH3, TAB3, RG)                                                                  \
    {                                                                                                           \
        {                                                                                                       \
            f32x2 cfv[NPL];                                                                                     \
            unsigned ofs[NPL];                                                                                  \
            WP_READ_C(CH2, cfv)                                                                                 \
            _Pragma("unroll") for (int sl = 0; sl < NPL; ++sl) ofs[sl] = sOff[((TAB3) * NPL + sl) * NT + tid];  \
            W3_WAIT(NA)                                                                                         \
            float pv[NPV];                                                                                      \
            _Pragma("unroll") for (int e = 0; e < NPV; ++e) pv[e] = 0.0f;                                       \
            W3_WRITE_P(par, min(Cin - (CH2) * CK, CK), pfl, pv, cfv)                                            \
            pfl = (ofs[0] & 1u) | ((ofs[1] & 1u) << 1) | ((ofs[2] & 1u) << 2);                                  \
            W3_LOAD_P(b, CH3, pv[0], ofs)                                                                       \
        }                                                                                                       \
        {                                                                                                       \
            f32x2 rw[3][4];                                                                                     \
            W3_READ_R((par) ^ 1, rw)                                                                            \
            W3_WRITE_V((par) ^ 1, RG, rw)                                                                       \
        }                                                                                                       \
    }

    f32x16 acc[2][COT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ct = 0; ct < COT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][ct][r] = 0.0f;

    // diagnostics (mcvd_ctx_set_debug_buffer): shader-clock time wave (a.wdma & 7) spends in {prologues, K loops, epilogues}
    const bool rec = a.dbg != nullptr && wave == (a.wdma & 7);
    unsigned long long tprev = t_start, dt[3] = {0, 0, 0}, rt0 = 0;
    if (rec) rt0 = __builtin_amdgcn_s_memrealtime();
#define WP_STAMP(i)                                                                                             \
    if (rec) {                                                                                                  \
        const unsigned long long now = __builtin_amdgcn_s_memtime();                                            \
        dt[i] += now - tprev;                                                                                   \
        tprev = now;                                                                                            \
    }

    const unsigned* const wpb_u = reinterpret_cast<const unsigned*>(a.wpb);
    const bool fin = ksp == 1;                 // K split: bias, residual and scale are applied by the reduce kernel
    int vtok = 0;                              // ordering token: written by every VMEM wait, an operand of the register reads
    unsigned pfl = 0;                          // zero-padding flags of the patch whose raw values are in flight (bit sl)
    int chunks_done = 0;

    int it = it0;
    while (it < it1) {
        // ================= a run: the items [it, run_end) of sample b =================
        const int b = it / ips;
        const int run_end = min(it1, (b + 1) * ips);
        // -------- prologue (conv_wino3.cpp).  Issue order = need order: the coefficients of the sample, the raw patches of the run's first
        // two chunks (into the registers of weight quads 0 .. PQ-1), the third patch, then the weight quads of the first chunk.
        {
            const int q0 = it - b * ips, kh = q0 % ksp, q1 = q0 / ksp, cotile = q1 % nct, rr = q1 / nct;
            const int oy0 = (rr / rx_n) * 8, ox0 = (rr % rx_n) * 16, cbeg = kh * nch;
            const unsigned* w0 = wpb_u + (((long)cotile * (nch * ksp) + cbeg) * 16 + 2 * wave_u) * (NQ * 256);
            const float* co_src[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) co_src[k] = a.coef + ((long)b * Cin + min(tid + k * NT, Cin - 1)) * 2;
            if (PRO)
                asm volatile("global_load_dwordx2 v[172:173], %0, off\n\tglobal_load_dwordx2 v[174:175], %1, off"
                             :: "v"(co_src[0]), "v"(co_src[1]) : "memory");
            const float nodep = 0.0f;
            unsigned ofs[NPL];
            WP_SLOT_TABLE(it & 1, oy0, ox0, ofs)
            const unsigned fl0 = (ofs[0] & 1u) | ((ofs[1] & 1u) << 1) | ((ofs[2] & 1u) << 2);
            W3_LOAD_PR(b, cbeg, nodep, ofs, "v[184:187]", "v[188:191]", "v192")
            W3_LOAD_PR(b, cbeg + 1, nodep, ofs, "v[194:197]", "v[198:201]", "v202")
            W3_WAIT(0)                         // the coefficients and the two patches have landed
            float cdep = 0.0f;
            if (PRO) {
                f32x2 cpre[2];
                asm volatile("v_mov_b32 %0, v172\n\tv_mov_b32 %1, v173\n\tv_mov_b32 %2, v174\n\tv_mov_b32 %3, v175"
                             : "=v"(cpre[0].x), "=v"(cpre[0].y), "=v"(cpre[1].x), "=v"(cpre[1].y) : "s"(vtok));
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (tid + k * NT < Cin) *reinterpret_cast<f32x2*>(sCo + (tid + k * NT) * 2) = cpre[k];
                cdep = cpre[0].x + cpre[1].x;
            }
            W3_LOAD_P(b, cbeg + 2, cdep, ofs)  // (behind the reads of v172-v175)
            pfl = fl0;
            if (PRO) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // coefficient table visible
            {
                // the weight quads PQ.. of the first chunk are requested one behind each activated value (conv_wino3.cpp)
                constexpr int QR = (NA - PQ + 2 * NPV - 1) / (2 * NPV);
#define WP_HOOK0(e, v) W3_LOAD_A_RANGE(w0, PQ + (e) * QR, (PQ + ((e) + 1) * QR < NA ? PQ + ((e) + 1) * QR : NA), v)
#define WP_HOOK1(e, v) W3_LOAD_A_RANGE(w0, (PQ + (NPV + (e)) * QR < NA ? PQ + (NPV + (e)) * QR : NA), (PQ + (NPV + (e) + 1) * QR < NA ? PQ + (NPV + (e) + 1) * QR : NA), v)
                float pv0[NPV], pv1[NPV];
                f32x2 cf0[NPL], cf1[NPL];
                WP_READ_C(cbeg, cf0)
                WP_READ_C(cbeg + 1, cf1)
                W3_WRITE_PR(0, min(Cin - cbeg * CK, CK), fl0, pv0, cf0, "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", WP_HOOK0)
                W3_WRITE_PR(1, min(Cin - (cbeg + 1) * CK, CK), fl0, pv1, cf1, "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", WP_HOOK1)
#undef WP_HOOK0
#undef WP_HOOK1
                const float dep = pv0[0] + pv1[0];
                W3_LOAD_A_RANGE(w0, 0, PQ, dep)
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");               // the first two patches visible
            {
                f32x2 rw[3][4];
                W3_READ_R(0, rw)
                W3_WRITE_V(0, rg, rw)
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");               // V of the first chunk visible
            W3_WAIT(0)                         // the loop's in-order counts start from an empty queue
        }
        WP_STAMP(0)
        int par = 0;                           // parity of the stream's current chunk: V(g) in sV[par], patch(g + 2) goes to sP[par]
        for (; it < run_end; ++it) {
            // ---- this item and the next one of the run (the stream stages up to three chunks of it; the last item of a run stages its
            // own first chunks once more: valid addresses, results never used)
            const int q0 = it - b * ips, kh = q0 % ksp, q1 = q0 / ksp, cotile = q1 % nct, rr = q1 / nct;
            const int nx = it + 1 < run_end ? it + 1 : it;
            const int n0 = nx - b * ips, nkh = n0 % ksp, n1 = n0 / ksp, ncotile = n1 % nct, nrr = n1 / nct;
            const int cbeg = kh * nch, ncbeg = nkh * nch;
            const unsigned* wb_cur = wpb_u + (((long)cotile * (nch * ksp) + cbeg) * 16 + 2 * wave_u) * (NQ * 256);
            const unsigned* wb_nx = wpb_u + (((long)ncotile * (nch * ksp) + ncbeg) * 16 + 2 * wave_u) * (NQ * 256);
            const int tab_cur = it & 1, tab_nx = nx & 1;
            {   // slot table of the next item (first read three chunks before this item ends; nch >= 4)
                unsigned dummy[NPL];
                WP_SLOT_TABLE(tab_nx, (nrr / rx_n) * 8, (nrr % rx_n) * 16, dummy)
                (void)dummy;
            }
            // VMEM issue order of a wave per chunk (in-order vmcnt counter; nothing else of the loop is outstanding):
            //   waves 0-3:  [patch(g+3): NPL loads] [weights(g+1): NQ loads behind the MFMAs of each position]      waves 4-7:  weights, then patch
            //   patch(g+2) before its write: vmcnt(NA); weights(g) of a position before its MFMAs: vmcnt(VM_A)       (conv_wino3.cpp)
#define WP_CHUNK_SCALARS                                                                                        \
            const int l2 = c + 2, l3 = c + 3;                                                                   \
            const int ch2 = l2 < nch ? cbeg + l2 : ncbeg + l2 - nch;                                            \
            const int ch3 = l3 < nch ? cbeg + l3 : ncbeg + l3 - nch;                                            \
            const int tab3 = l3 < nch ? tab_cur : tab_nx;                                                       \
            const unsigned* wnx = c + 1 < nch ? wb_cur + (long)(c + 1) * WSTR : wb_nx;
            if (rg == 0) {
                for (int c = 0; c < nch; ++c) {
                    WP_CHUNK_SCALARS
                    WP_VALU_PHASE(par, ch2, ch3, tab3, rg)
                    W3_MFMA_PHASE(par, true, wnx)
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    par ^= 1;
                }
                // the loads still in flight target registers the compiler does not know: one wait behind each loop (two different asm
                // texts: identical statements would be sunk into the join block, behind code the checker cannot see through)
                asm volatile("s_waitcnt vmcnt(0) ; staging-first loop left" ::: "memory");
            } else {
                for (int c = 0; c < nch; ++c) {
                    WP_CHUNK_SCALARS
                    W3_MFMA_PHASE(par, true, wnx)
                    WP_VALU_PHASE(par, ch2, ch3, tab3, rg)
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    par ^= 1;
                }
                asm volatile("s_waitcnt vmcnt(0) ; matrix-first loop left" ::: "memory");
            }
#undef WP_CHUNK_SCALARS
            chunks_done += nch;
            // The MFMAs are inline asm: the compiler inserts none of the wait states a read of an MFMA result needs (8-pass MFMA -> VALU /
            // LDS read: 11).  The nops are tied to the accumulators.
            if constexpr (COT == 3)
                asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]) :: "memory");
            else if constexpr (COT == 2)
                asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]) :: "memory");
            else
                asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0][0]), "+v"(acc[1][0]) :: "memory");
            WP_STAMP(1)

            // ---------------- inverse transform + epilogue of the item, one 32-cout sub-tile per round ----------------
            // LDS: 64 KiB of position planes [16][32 couts][32 tiles] in what the stream has just vacated -- positions 0-11 in the V buffer of
            // the item's last chunk (par was flipped behind it: sV[par ^ 1], 48 KiB), positions 12-15 in the patch buffer whose chunk was
            // transformed during that last iteration (sP[par], 16 KiB).  The other V buffer and the other patch buffer hold the next item's
            // first chunks.  (A first form had 32 KiB only and ran six rounds of 16 couts: twice the barriers, one task per thread and round.)
            float* sM0 = smem + ((par ^ 1) ? VW : 0);                 // positions 0 .. 11
            float* sM1 = sP + (par ? PBUF : 0);                       // positions 12 .. 15
            // the epilogue's thread indices are recomputed per item from an opaque copy of tid: hoisted out of the item loop they would be
            // live across the K loops, whose register budget is the accumulators' (the allocator spilled them to scratch)
            int tid_e;
            asm volatile("v_mov_b32 %0, %1" : "=v"(tid_e) : "v"(tid));
            const int e_tile = tid_e & 31, e_col0 = tid_e >> 5;      // two (cout, tile) tasks per thread and round: couts e_col0 and e_col0 + 16
            const int e_ty = e_tile >> 3, e_tx = e_tile & 7;
            const int oy0 = (rr / rx_n) * 8, ox0 = (rr % rx_n) * 16, co0 = cotile * BCO;
            const long pix = (long)(oy0 + 2 * e_ty) * W + ox0 + 2 * e_tx;
            float* const ydst = fin ? a.y : a.part + (long)kh * a.B * a.Cout * HW;
            // bias and residual of a round are requested one round ahead (fetched where they are used, every round waited for two
            // dependent memory latencies between its barriers; all 2 * COT tasks up front do not fit beside the accumulators here)
            float e_bias[COT][2];
            f32x2 e_r0[COT][2], e_r1[COT][2];
#define WP_EPI_FETCH(ct)                                                                                        \
            {                                                                                                   \
                _Pragma("unroll") for (int t2 = 0; t2 < 2; ++t2) {                                              \
                    const int co = co0 + (ct) * 32 + e_col0 + 16 * t2;                                          \
                    e_bias[ct][t2] = fin ? a.bias[co] : 0.0f;           /* zero-padded to CoutP */               \
                    e_r0[ct][t2] = e_r1[ct][t2] = f32x2{0.0f, 0.0f};                                            \
                    if (a.res && fin) {                                                                         \
                        const long o = ((long)b * a.Cout + min(co, a.Cout - 1)) * HW + pix;                     \
                        e_r0[ct][t2] = *reinterpret_cast<const f32x2*>(a.res + o);                              \
                        e_r1[ct][t2] = *reinterpret_cast<const f32x2*>(a.res + o + W);                          \
                    }                                                                                           \
                }                                                                                               \
            }
            WP_EPI_FETCH(0)
            float* const sMw = wave_u < 6 ? sM0 + (2 * wave_u) * (32 * T) : sM1 + (2 * wave_u - 12) * (32 * T);      // this wave's two planes
#pragma unroll
            for (int ct = 0; ct < COT; ++ct) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int col = (r & 3) + 8 * (r >> 2) + 4 * half;
                        sMw[(i * 32 + col) * T + l31] = acc[i][ct][r];
                    }
                if (ct + 1 < COT) WP_EPI_FETCH(ct + 1 < COT ? ct + 1 : ct)
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    const int e_col = e_col0 + 16 * t2;
                    const int co = co0 + ct * 32 + e_col;
                    WINO_EPILOGUE_TASK(false, true, sM0, sM1, 1.0f, e_bias[ct][t2], e_r0[ct][t2], e_r1[ct][t2], b, true, rpi, rr)
                }
                // the round's LDS reads done before the next round's writes -- and, behind the last round, before the stream's next
                // park / transform write into these buffers
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            // the accumulators of the next item start from zero (VALU writes; the first MFMA that reads them is hundreds of cycles away)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int ct = 0; ct < COT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][ct][r] = 0.0f;
            WP_STAMP(2)
        }
        // end of the run: every asm load has landed (vmcnt(0) behind the last K loop), the epilogue's last barrier has passed
    }
    if (rec) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            unsigned long long* d = a.dbg + (long)blockIdx.x * 8;
            unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            d[0] = dt[0]; d[1] = dt[1]; d[2] = rt0; d[3] = __builtin_amdgcn_s_memrealtime();
            d[4] = ((unsigned long long)xcc << 32) | hwid;
            d[5] = dt[2];                  // epilogues
            d[6] = (unsigned long long)chunks_done | ((unsigned long long)(it1 - it0) << 32);
            d[7] = now - t_start;
        }
    }
#undef WP_STAMP
#undef WP_EPI_FETCH
#undef WP_SLOT_TABLE
#undef WP_READ_C
#undef WP_VALU_PHASE
#undef W3_SLOT_OFF
#undef W3_TS
#define W3_STAGE_UNDEF
#include "conv_wino3_stage.h"
}

static constexpr size_t wino3p_lds_bytes(int Cin) {
    return (size_t)(2 * W3_VW + 2 * 4096 + 2 * Cin + 2 * WP_NPL * W3_NT) * sizeof(float);
}
static_assert(wino3p_lds_bytes(WINO_TABLE_CH) == 151552 && wino3p_lds_bytes(WINO_TABLE_CH) <= 160 * 1024,
              "the widest table the rule admits (conv_kernels.h: kWinoRules, all Cin <= WINO_TABLE_CH channels) fits the LDS: no LDS term in the rule");

// compute units of the current device (one persistent workgroup each), cached per device
static int wino3p_num_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cus[dev].load(std::memory_order_acquire);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev].store(n, std::memory_order_release);
    return n;
}

template <int COT, int PRO>
static int wino3p_launch2(const ConvArgs& a, hipStream_t s) {
    constexpr int BCO = 32 * COT;
    const int ksp = a.ksplit >= 2 ? a.ksplit : 1;
    const long n_items = (long)a.B * (a.H / 8) * (a.W / 16) * (a.CoutP / BCO) * ksp;
    const int cus = a.pgrid > 0 ? a.pgrid : wino3p_num_cus();
    dim3 grid((unsigned)(n_items < cus ? n_items : cus));
    ConvArgs k = a;
    if (k.dbg) k.wdma = 0;                 // wave 0 records its phase times
#ifdef MCVD_DIAG
    if (k.dbg) {
        const char* w = getenv("MCVD_DBG_WAVE");
        k.wdma = w ? atoi(w) : 0;
    }
    k.wdma &= 0xff;
    if (const char* st = getenv("MCVD_W3P_STAGGER")) k.wdma |= atoi(st) << 8;
#else
    k.wdma &= 0xff;
#endif
    if (int rc = wino_launch_kernel<conv_wino3p_kernel<COT, PRO>>(k, grid, W3_NT, wino3p_lds_bytes(a.Cin), s)) return rc;
    return wino_launch_done(a, false, ksp, s);
}

// Shape ids 16 / 17 / 20: regions of 8 x 16 output pixels only, at least WP_MINCH chunks per item, all Cin channels in one table (the rule's row
// says why it stops at WINO_TABLE_CH); wider layers take the one-shot kernel (ids 11 / 18 / 19).
int launch_conv_wino3p(const ConvArgs& a, hipStream_t s) {
    static_assert(wino_rule(CF_WINO3P)->chunk == W3_CK && wino_rule(CF_WINO3P)->min_chunks[0] == WP_MINCH && wino_rule(CF_WINO3P)->min_chunks[3] == WP_MINCH,
                  "the rule's chunk and the fewest chunks of an item are the kernel's");
    if (int rc = conv_wino_require(CF_WINO3P, a, "persistent winograd bf16x3 conv")) return rc;
    const int cot = conv_wino_cout_tile(a.Cout);
    MCVD_REQUIRE(a.CoutP % (32 * cot) == 0, "persistent winograd bf16x3 conv: CoutP=%d vs tile %d", a.CoutP, 32 * cot);
    return wino_dispatch(a, cot, [&](auto COT, auto PRO, auto) { return wino3p_launch2<COT(), PRO()>(a, s); });
}

}  // namespace mcvd
