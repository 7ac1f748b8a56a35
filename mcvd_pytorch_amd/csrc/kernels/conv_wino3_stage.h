// The K-loop stage of the two three-piece bf16 Winograd kernels, conv_wino3_kernel (conv_wino3.cpp: one workgroup per region and
// cout tile) and conv_wino3p_kernel (conv_wino3p.cpp: persistent workgroups): ONE text, so the two K loops are the same
// instruction sequence by construction (tests/test_gpu_wino3p.py holds their results bit-identical).  The shared constants, the
// named-register map and the macros that load, park, transform and multiply one chunk; each kernel keeps what is its own -- the
// chunk loop or the item stream, the coefficient table's index (W3_READ_C / WP_READ_C), its VALU phase, the prologue's order, the epilogue.
//
// Included twice by each file: in front of its kernel, and behind it with W3_STAGE_UNDEF defined (the #undef list).
//
// The macros expand inside the kernel and use its names:
//   constexpr  COT, PRO, G8, EXP (conv_wino3p.cpp: G8 = false, EXP = 0 -- those branches vanish), CK, T, PP, PW, VW, PBUF, NPL, NPV,
//              NQ, VM_A
//   values     a (ConvArgs), Cin, HW, wave, half, l31, wr_voff (lane * 16), p_pk[NPL], p_rd, v_wr, sV, sP, vtok, acc[2][COT]
//   macros     W3_SLOT_OFF(word): byte offset in a word of the patch-slot table; W3_TS(i): a clock stamp of the diagnostics build, or nothing
// Arguments: `par` the parity of the V / patch buffer, `bb` the sample, `ch` the absolute chunk, WPTR / WNX the wave's weights of a
// chunk: its 2 * NQ quads, quad q = (i * COT + ct) * 3 + piece of positions 2w + i, 256 dwords each.
#ifdef W3_STAGE_UNDEF
#undef W3_QUADS
#undef W3_LD1
#undef W3_LD1D
#undef W3_MF1
#undef W3_LOAD_A
#undef W3_LOAD_A_PIECE
#undef W3_LOAD_A_RANGE
#undef W3_WAIT
#undef W3_LOAD_PR
#undef W3_LOAD_P
#undef W3_NOHOOK
#undef W3_WRITE_PR
#undef W3_WRITE_P
#undef W3_READ_R
#undef W3_WRITE_V
#undef W3_LOAD_B
#undef W3_PRODUCT
#undef W3_MFMA_PHASE
#undef W3_STAGE_UNDEF
#else

#include "wino_common.h"

namespace mcvd {

constexpr int W3_CK = 16;        // input channels per chunk = K of one bf16 MFMA
constexpr int W3_T = 32;         // tiles per workgroup / item (4 x 8 tiles = 8 x 16 output pixels)
constexpr int W3_NT = 512;
#ifndef MCVD_W3_PP
#define MCVD_W3_PP 24
#endif
// LDS patch row pitch in channel-pair columns (18 used; 20 for the two 8x8 images side by side).  The patch park stores a lane's four pixels as
// single dwords at ((pair * 10 + row) * PP + col) * 2 + ce; the 32 lanes of a store group are 8 rows x 4 four-pixel items, bank = (row * 2 PP +
// 8 item) mod 32: with 2 PP = 48 = 16 (mod 32) they fall on FOUR banks -- the "x4 patch park" conflict behind 27-29 percent of the LDS-active
// cycles (profiles/r04_pmc_sq_wave_states.txt).  Round 5 built the conflict-free pitch (25: 2 PP = 18 mod 32, 16 banks, 2-way = free for
// ds_write_b32) and measured it against 24 on one box (tools/build_variant.sh, -DMCVD_W3_PP=25; profiles/r05_patch_pitch_ab.txt): 5577 vs 5592
// cycles per chunk, 248.1 / 248.5 vs 248.8 / 249.4 frames/s -- nothing.  The stores are not on the chunk's critical path; 24 stays.
constexpr int W3_PP = MCVD_W3_PP;
constexpr int W3_PW = 16 * 2 * 4 * W3_T;          // 32-bit words of one piece plane of a V chunk: [position][half][pair][tile]
constexpr int W3_VW = 3 * W3_PW;                  // 32-bit words of one V chunk: [piece][position][half][pair][tile]

}  // namespace mcvd

/* IN-FLIGHT DATA LIVES IN REGISTERS THE COMPILER DOES NOT ALLOCATE.  The kernels are compiled with amdgpu_num_vgpr(86): v172-v255 are
   never touched by generated code.  The asm loads write them (weight quad q: v[184 + 4q : 187 + 4q]; patch slots: v[172:175], v[176:179], v180), the
   waits are bare s_waitcnt, the MFMAs name their A operand in the instruction text.  (Loads whose results are compiler-visible
   values are not safe here: the register allocator may assign the result and the operand of the later wait to different registers
   and copy between them while the load is still in flight -- it did, a wrong result once in ~10^4 launches.)
   Every statement that touches a named register is `asm volatile` (program order among them is kept) except the patch FMAs, which
   take the wait's token (an SGPR) as an operand. */
#define W3_QUADS(X, q, A1, A2) X(0, "v[184:187]", q, A1, A2) X(1, "v[188:191]", q, A1, A2) X(2, "v[192:195]", q, A1, A2) X(3, "v[196:199]", q, A1, A2) X(4, "v[200:203]", q, A1, A2) X(5, "v[204:207]", q, A1, A2) X(6, "v[208:211]", q, A1, A2) X(7, "v[212:215]", q, A1, A2) X(8, "v[216:219]", q, A1, A2) X(9, "v[220:223]", q, A1, A2) X(10, "v[224:227]", q, A1, A2) X(11, "v[228:231]", q, A1, A2) X(12, "v[232:235]", q, A1, A2) X(13, "v[236:239]", q, A1, A2) X(14, "v[240:243]", q, A1, A2) X(15, "v[244:247]", q, A1, A2) X(16, "v[248:251]", q, A1, A2) X(17, "v[252:255]", q, A1, A2)
#define W3_LD1(K, R, q, P, UNUSED) if ((q) == K) asm volatile("global_load_dwordx4 " R ", %0, %1" :: "v"(wr_voff), "s"(P) : "memory");
#define W3_MF1(K, R, q, ACC, BV) if ((q) == K) asm volatile("v_mfma_f32_32x32x16_bf16 %0, " R ", %1, %0" : "+v"(ACC) : "v"(BV));
/* the NQ weight quads of position 2w + i */
#define W3_LOAD_A(WPTR, i)                                                                                      \
    {                                                                                                           \
        const unsigned* ua = (WPTR) + (i) * (NQ * 256);                                                         \
        _Pragma("unroll") for (int qq = 0; qq < NQ; ++qq) { W3_QUADS(W3_LD1, (i) * NQ + qq, ua + qq * 256, 0) } \
    }
/* weight piece `pc` of every cout sub-tile of position 2w + i (quads (i * COT + ct) * 3 + pc) */
#define W3_LOAD_A_PIECE(WPTR, i, pc)                                                                            \
    {                                                                                                           \
        const unsigned* ua = (WPTR) + (i) * (NQ * 256);                                                         \
        _Pragma("unroll") for (int ct = 0; ct < COT; ++ct) { W3_QUADS(W3_LD1, (i) * NQ + ct * 3 + (pc), ua + (ct * 3 + (pc)) * 256, 0) } \
    }
/* prologue: quads Q0 .. Q1-1, issued behind the instructions that produced DEP (which read the registers) */
#define W3_LD1D(K, R, q, P, DEP) if ((q) == K) asm volatile("global_load_dwordx4 " R ", %0, %1" :: "v"(wr_voff), "s"(P), "v"(DEP) : "memory");
#define W3_LOAD_A_RANGE(WPTR, Q0, Q1, DEP)                                                                      \
    {                                                                                                           \
        const unsigned* ua = (WPTR);                                                                            \
        _Pragma("unroll") for (int qq = (Q0); qq < (Q1); ++qq) { W3_QUADS(W3_LD1D, qq, ua + qq * 256, DEP) }    \
    }
#define W3_WAIT(N) asm volatile("s_waitcnt vmcnt(%1)\n\ts_mov_b32 %0, 0" : "=s"(vtok) : "n"(N) : "memory");
/* unconditional, clamped raw loads of the patch of chunk `ch` of sample `bb`: OFS = the slots' table words, RA / RB = the two
   four-pixel slots, RH = the halo slot; DEP = a value computed from the previous contents of those registers (ordering) */
#define W3_LOAD_PR(bb, ch, DEP, OFS, RA, RB, RH)                                                                \
    {                                                                                                           \
        const int cb = min((ch) * CK, Cin - 1);                                                                 \
        const unsigned lim4 = (unsigned)((Cin - cb) * HW - 4) * 4u, lim1 = (unsigned)((Cin - cb) * HW - 1) * 4u; \
        const bool second = cb >= a.C0;                                                                         \
        const float* srcb = second ? a.x1 + ((long)(bb) * a.C1 + (cb - a.C0)) * HW : a.x0 + ((long)(bb) * a.C0 + cb) * HW; \
        /* channels past the last one are zeroed at the write: any (aligned) address inside the source will do */ \
        if constexpr (G8) {                                                                                     \
            const unsigned istride = (unsigned)((second ? a.C1 : a.C0) * HW) * 4u;      /* distance to the region's second sample */ \
            const unsigned o0 = min(W3_SLOT_OFF(OFS[0]), lim4) + ((p_pk[0] >> 20) & 1u) * istride;              \
            asm volatile("global_load_dwordx4 " RA ", %0, %1" :: "v"(o0), "s"(srcb), "v"(DEP) : "memory");     \
        } else {                                                                                                \
            const unsigned o0 = min(W3_SLOT_OFF(OFS[0]), lim4), o1 = min(W3_SLOT_OFF(OFS[NPL > 1 ? 1 : 0]), lim4),  \
                           o2 = min(W3_SLOT_OFF(OFS[NPL > 2 ? 2 : 0]), lim1);                                   \
            asm volatile("global_load_dwordx4 " RA ", %0, %3\n\tglobal_load_dwordx4 " RB ", %1, %3\n\tglobal_load_dword " RH ", %2, %3" \
                         :: "v"(o0), "v"(o1), "v"(o2), "s"(srcb), "v"(DEP) : "memory");                           \
        }                                                                                                       \
    }
#define W3_LOAD_P(bb, ch, DEP, OFS) W3_LOAD_PR(bb, ch, DEP, OFS, "v[172:175]", "v[176:179]", "v180")
#define W3_NOHOOK(e, v)
#define W3_WRITE_P(par, NV, FL, PV, cfv) W3_WRITE_PR(par, NV, FL, PV, cfv, "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", W3_NOHOOK)
/* activate once per pixel (coefficients cfv: one pair per slot, a slot is one channel) and park a chunk's patch in patch buffer
   `par`; NV = the chunk's channels that exist, Cin - ch * CK (more than CK is as good as CK; evaluated in front of the FMAs: the
   persistent kernel passes it clamped, the one-shot kernel as it is, and each K loop is scheduled as it was around that); FL bit sl =
   slot sl is zero padding (as is a slot whose channel code is CK or more); zero padding applies AFTER the activation.
   HOOK(e, v): statements placed behind value e (the prologues issue their weight loads there, one at a time) */
#define W3_WRITE_PR(par, NV, FL, PV, cfv, A0, A1, A2, A3, B0, B1, B2, B3, H0, HOOK)                             \
    {                                                                                                           \
        float* sPw = sP + ((par) ? PBUF : 0);                                                                   \
        const int nvalid = (NV);                                                                                \
        /* v = A * raw + B straight out of the patch registers (PRO 0: A = 1, B = 0, exact): the only reads of those registers */ \
        if constexpr (G8) {                                                                                     \
            asm("v_fma_f32 %0, " A0 ", %4, %5\n\tv_fma_f32 %1, " A1 ", %4, %5\n\tv_fma_f32 %2, " A2 ", %4, %5\n\tv_fma_f32 %3, " A3 ", %4, %5" \
                : "=&v"(PV[0]), "=&v"(PV[1]), "=&v"(PV[2]), "=&v"(PV[3]) : "v"(cfv[0].x), "v"(cfv[0].y), "s"(vtok)); \
        } else {                                                                                                \
            asm("v_fma_f32 %0, " A0 ", %9, %10\n\tv_fma_f32 %1, " A1 ", %9, %10\n\tv_fma_f32 %2, " A2 ", %9, %10\n\tv_fma_f32 %3, " A3 ", %9, %10\n\t" \
                "v_fma_f32 %4, " B0 ", %11, %12\n\tv_fma_f32 %5, " B1 ", %11, %12\n\tv_fma_f32 %6, " B2 ", %11, %12\n\tv_fma_f32 %7, " B3 ", %11, %12\n\t" \
                "v_fma_f32 %8, " H0 ", %13, %14"                                                                  \
                : "=&v"(PV[0]), "=&v"(PV[1]), "=&v"(PV[2]), "=&v"(PV[3]), "=&v"(PV[4]), "=&v"(PV[5]), "=&v"(PV[6]), "=&v"(PV[7]), "=&v"(PV[NPV > 8 ? 8 : 0]) \
                : "v"(cfv[0].x), "v"(cfv[0].y), "v"(cfv[NPL > 1 ? 1 : 0].x), "v"(cfv[NPL > 1 ? 1 : 0].y), "v"(cfv[NPL > 2 ? 2 : 0].x), \
                  "v"(cfv[NPL > 2 ? 2 : 0].y), "s"(vtok));                                                        \
        }                                                                                                       \
        _Pragma("unroll") for (int e = 0; e < NPV; ++e) {                                                       \
            const int sl = e >> 2;                            /* values 0-3: slot 0, 4-7: slot 1, 8: slot 2 */   \
            float v = PV[e];                                                                                    \
            if (PRO >= 2) v = wino_silu(v);                                                                     \
            const bool keep = (((FL) >> sl) & 1u) == 0u && (int)((p_pk[sl] >> 12) & 0xff) < min(nvalid, CK);    \
            sPw[(p_pk[sl] & 0xfff) + 2 * (e & 3)] = keep ? v : 0.0f;                                            \
            HOOK(e, v)                                                                                          \
        }                                                                                                       \
    }
/* rows 2rg and 2rg+1 of B^T d for the two channels of the pair (packed fp32: .x = channel s_ca, .y = s_ca + 2), (.) B,
   three-way bf16 split, 24 stores:
   row 0: d0 - d2   row 1: d1 + d2   row 2: d2 - d1   row 3: d1 - d3;   (.) B: m0 - m2, m1 + m2, m2 - m1, m1 - m3 */
#define W3_READ_R(par, RW)                                                                                      \
    {                                                                                                           \
        const f32x2* sPr = reinterpret_cast<const f32x2*>(sP + ((par) ? PBUF : 0) + p_rd);                      \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) { RW[0][j] = sPr[j]; RW[1][j] = sPr[PP + j]; RW[2][j] = sPr[2 * PP + j]; } \
    }
#define W3_WRITE_V(par, RG, RW)                                                                                 \
    {                                                                                                           \
        unsigned* vdst = sV + ((par) ? VW : 0) + v_wr;                                                          \
        f32x2 mx[4], my[4];                                                                                     \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                         \
            const f32x2 r0 = RW[0][j], r1 = RW[1][j], r2 = RW[2][j];                                            \
            if ((RG) == 0) { mx[j] = r0 - r2; my[j] = r1 + r2; }                                                \
            else { mx[j] = r1 - r0; my[j] = r0 - r2; }                                                          \
        }                                                                                                       \
        _Pragma("unroll") for (int row = 0; row < 2; ++row) {                                                   \
            const f32x2 m0 = row ? my[0] : mx[0], m1 = row ? my[1] : mx[1], m2 = row ? my[2] : mx[2], m3 = row ? my[3] : mx[3]; \
            const f32x2 v0 = m0 - m2, v1 = m1 + m2, v2 = m2 - m1, v3 = m1 - m3;                                 \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                     \
                unsigned w1, w2, w3;                                                                            \
                wino_split3(q == 0 ? v0 : q == 1 ? v1 : q == 2 ? v2 : v3, w1, w2, w3);                          \
                vdst[(row * 4 + q) * 256] = w1;                                                                 \
                vdst[(row * 4 + q) * 256 + PW] = w2;                                                            \
                vdst[(row * 4 + q) * 256 + 2 * PW] = w3;                                                        \
            }                                                                                                   \
        }                                                                                                       \
    }
/* B operand of position 2w+i -> BQ[piece][pair]  <-  word (((p*16 + pos)*2 + half)*4 + jp)*T + l31 of the V chunk at sVc */
#define W3_LOAD_B(i, BQ)                                                                                        \
    {                                                                                                           \
        const unsigned* q = sVc + (((2 * wave + (i)) * 2 + half) * 4) * T + l31;                                \
        _Pragma("unroll") for (int jp = 0; jp < 4; ++jp) {                                                      \
            BQ[0][jp] = q[jp * T]; BQ[1][jp] = q[PW + jp * T]; BQ[2][jp] = q[2 * PW + jp * T];                  \
        }                                                                                                       \
    }
/* the COT MFMAs of one piece product (weight piece PA x activation piece PB) of position 2w + i */
#define W3_PRODUCT(i, PA, PB)                                                                                   \
    { _Pragma("unroll") for (int ct = 0; ct < COT; ++ct) { W3_QUADS(W3_MF1, 3 * ((i) * COT + ct) + (PA), acc[i][ct], bq[i][PB]) } }
/* all MFMAs of the chunk whose V sits in buffer `par` (its weights in the named registers).  Per position 2w + i: wait for its NQ
   quads, 6*COT MFMAs ordered product-major (u3 v1, u2 v2, u1 v3, u2 v1, u1 v2, u1 v1: smallest class first; consecutive MFMAs write
   different accumulators), and -- NEXT -- the same NQ quads are reloaded piece by piece from WNX, the (wave's) weights of the next
   chunk (the matrix pipe has read its A operands by the time the wave gets past the MFMA: it issues in order).  In-order VMEM
   bookkeeping: when the quads of a position are needed, the loads issued after them are the other position's NQ quads and one
   patch group: vmcnt(NQ + NPL) = VM_A, in both phase orders. */
#define W3_MFMA_PHASE(par, NEXT, WNX)                                                                           \
    {                                                                                                           \
        const unsigned* sVc = sV + ((par) ? VW : 0);                                                            \
        u32x4 bq[2][3];                                                                                         \
        W3_TS(7)                                                                                                \
        if (!(EXP & 8)) { W3_LOAD_B(0, bq[0]) W3_LOAD_B(1, bq[1]) }                                             \
        else { _Pragma("unroll") for (int p = 0; p < 3; ++p) { bq[0][p] = u32x4{1, 2, 3, 4}; bq[1][p] = u32x4{5, 6, 7, 8}; } } \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                         \
            if (NEXT && !(EXP & 4)) W3_WAIT(VM_A)                                                               \
            if (!(EXP & 16)) {                                                                                  \
                /* a weight piece is re-requested for the next chunk as soon as its LAST product has been issued: u3 behind the first \
                   product, u2 behind the fourth, u1 behind the sixth -- three requests at a time, spread over the position's 576   \
                   cycles of matrix work (nine in one burst stall the wave in the issue: the CU's vector-memory path is 70 % busy) */ \
                W3_PRODUCT(i, 2, 0)                                                                             \
                if (NEXT && !(EXP & 4)) W3_LOAD_A_PIECE(WNX, i, 2)                                              \
                W3_PRODUCT(i, 1, 1) W3_PRODUCT(i, 0, 2) W3_PRODUCT(i, 1, 0)                                     \
                if (NEXT && !(EXP & 4)) W3_LOAD_A_PIECE(WNX, i, 1)                                              \
                W3_PRODUCT(i, 0, 1) W3_PRODUCT(i, 0, 0)                                                         \
                if (NEXT && !(EXP & 4)) W3_LOAD_A_PIECE(WNX, i, 0)                                              \
            } else {                                                                                            \
                _Pragma("unroll") for (int ct = 0; ct < COT; ++ct)                                              \
                    acc[i][ct][0] += __builtin_bit_cast(float, bq[i][0][0] ^ bq[i][1][1] ^ bq[i][2][2] ^ bq[i][1][3]); \
                if (NEXT && !(EXP & 4)) W3_LOAD_A(WNX, i)                                                       \
            }                                                                                                   \
            W3_TS(4 + i)                                                                                        \
        }                                                                                                       \
    }
#endif
