// The attention kernels, once: which one a launch takes.  The numbers are public (mcvd_last_attention_kernel / mcvd_model_op_attention_kernel,
// profiles/): a new kernel gets a new number; numbers are never reused.
// Plain C++17, no HIP: the static_asserts at the end check the table in every build.
#pragma once

namespace mcvd {

enum AttnKernel : int {
    AK_NAIVE = 0,              // one thread per query, three passes: every shape (attention.cpp)
    AK_FLASH_F32 = 1,          // flash kernel on the fp32 MFMA: head dims 32 ... 256 (attention.cpp)
    AK_SPLIT2 = 2,             // flash kernel on the fp16 pipe, two-piece operands: head dims 32 ... 128 (attention_h2.cpp, NP = 2)
    AK_SPLIT3 = 3,             // ... on the bf16 pipe, three-piece operands, fp32-equivalent (attention_h2.cpp, NP = 3)
    AK_SPLIT3_PRESPLIT = 4,    // ... fed with K / V pre-split by the q|k|v projection; chosen by the model in place of AK_SPLIT3, bit-identical to it
    AK_WIDE2 = 5,              // head dim divided over the waves, two-piece fp16 operands: head dims 160 ... 1024 (attention_wide.cpp, NP = 2)
    AK_WIDE3 = 6               // ... three-piece bf16 operands, fp32-equivalent (attention_wide.cpp, NP = 3)
};

constexpr int AK_SPLIT_D_MAX = 128;        // attention_h2.cpp: Q pieces + O accumulators of a whole head in one lane
constexpr int AK_F32_D_MAX = 256;          // attention.cpp's flash kernel
constexpr int AK_WIDE_D_MIN = 160, AK_WIDE_D_MAX = 1024;
// 128 < D <= 256 has two kernels, the wide one and the fp32 flash kernel: the verdict of tools/attn_wide_time.py on D = 160, 192, 224, 256 x
// HW = 64, 256, 1024 at B * heads = 64 (profiles/attn_wide_time.txt).  Every D of the band gave the same answer:
//   three pieces: the wide kernel wins at HW = 64 (x 1.6 ... 1.9) and 256 (x 1.3 ... 1.5) and loses at 1024 (D = 160 / 192 / 256: x 0.85 / 0.88 /
//                 0.91; 224 was measured there with the first build of the kernel only, x 0.57 like its neighbours then.  Its waves repeat
//                 the softmax of a 32-query tile; the fp32 kernel's workgroup has 128 queries) -> wide up to AK_WIDE3_BAND_HW_MAX tokens.
//                 Token counts between 256 and 1024 and above 1024 were not measured: they follow the 1024 verdict;
//   two pieces:   the wide kernel wins at every measured HW (x 1.2 ... 2.2) -> wide at every token count.
// Above 256 the wide kernel has no rival but AK_NAIVE (x 325 ... 1700 measured).
constexpr int AK_WIDE_FROM_D = 160;
constexpr int AK_WIDE3_BAND_HW_MAX = 256;

// mode = the "naive_attn" option: 0 auto (the two-piece kernels when f16x2 is on, else the three-piece ones when bf16x3 is on, where one
// applies; else as 2), 1 the one-thread-per-query kernel, 2 the fp32 flash kernel where it applies, else the one-thread-per-query
// kernel (the dispatch before the wide kernel existed), 3 the two-piece kernels where one applies, 4 the three-piece kernels where one
// applies (3 / 4 elsewhere: as 2).  A head dim or a token count that is no multiple of 32 runs AK_NAIVE.
constexpr AttnKernel attn_kernel_for(int mode, int f16x2, int bf16x3, int C, int heads, int HW) {
    if (mode == 1 || heads <= 0 || C <= 0 || C % heads != 0) return AK_NAIVE;
    const int D = C / heads;
    if (D % 32 != 0 || HW <= 0 || HW % 32 != 0) return AK_NAIVE;
    const int np = (mode == 3 || (mode == 0 && f16x2)) ? 2 : (mode == 4 || (mode == 0 && bf16x3)) ? 3 : 0;
    if (np && D <= AK_SPLIT_D_MAX) return np == 2 ? AK_SPLIT2 : AK_SPLIT3;
    const bool band = D >= AK_WIDE_FROM_D && (np == 2 || HW <= AK_WIDE3_BAND_HW_MAX);          // 128 < D <= 256: the measured verdict
    if (np && D >= AK_WIDE_D_MIN && D <= AK_WIDE_D_MAX && (D > AK_F32_D_MAX || band)) return np == 2 ? AK_WIDE2 : AK_WIDE3;
    return D <= AK_F32_D_MAX ? AK_FLASH_F32 : AK_NAIVE;
}

// ---- the table, checked ----
namespace attn_kernels_check {
// what launch_attention's `if` chain ran before this header existed (head dims up to 128 must not move)
constexpr AttnKernel before(int mode, int f16x2, int bf16x3, int D) {
    if (mode == 1) return AK_NAIVE;
    if (D <= 128 && (mode == 3 || (mode == 0 && f16x2))) return AK_SPLIT2;
    if (D <= 128 && (mode == 4 || (mode == 0 && bf16x3))) return AK_SPLIT3;
    return D <= 256 ? AK_FLASH_F32 : AK_NAIVE;
}
// every D in 32 ... 1024 step 32 at HW = 64, every mode and option pair: one kernel, of the arithmetic the mode names, serving that D
constexpr bool table_sound() {
    for (int D = 32; D <= 1024; D += 32)
        for (int mode = 0; mode <= 4; ++mode)
            for (int opt = 0; opt < 4; ++opt) {
                const int f = opt & 1, b3 = opt >> 1;
                const AttnKernel k = attn_kernel_for(mode, f, b3, D, 1, 64);
                if (k != attn_kernel_for(mode, f, b3, 3 * D, 3, 64)) return false;                  // the head dim decides, not C
                if (D <= 128 && k != before(mode, f, b3, D)) return false;
                if ((mode == 1 || mode == 2) && k != before(mode, f, b3, D)) return false;          // the comparison legs never move
                const int np = (mode == 3 || (mode == 0 && f)) ? 2 : (mode == 4 || (mode == 0 && b3)) ? 3 : 0;
                if (np == 0 && k != before(mode, f, b3, D)) return false;
                if (np && D > 256 && k != (np == 2 ? AK_WIDE2 : AK_WIDE3)) return false;
                if (np && D > 128 && D <= 256 && k != AK_FLASH_F32 && k != (np == 2 ? AK_WIDE2 : AK_WIDE3)) return false;
                if (k == AK_SPLIT3_PRESPLIT) return false;                                          // the model's choice, never the table's
                if ((k == AK_WIDE2 || k == AK_WIDE3) && (D < AK_WIDE_D_MIN || D > AK_WIDE_D_MAX)) return false;
                if (k == AK_FLASH_F32 && D > AK_F32_D_MAX) return false;
                if ((k == AK_SPLIT2 || k == AK_SPLIT3) && D > AK_SPLIT_D_MAX) return false;
            }
    return true;
}
static_assert(table_sound(), "attention dispatch: a head dim without exactly one kernel of the arithmetic its mode names, or a D <= 128 row that moved");
static_assert(AK_NAIVE == 0 && AK_FLASH_F32 == 1 && AK_SPLIT2 == 2 && AK_SPLIT3 == 3 && AK_SPLIT3_PRESPLIT == 4 && AK_WIDE2 == 5 && AK_WIDE3 == 6,
              "the public numbers");
static_assert(attn_kernel_for(0, 0, 1, 384, 1, 64) == AK_WIDE3 && attn_kernel_for(0, 1, 1, 384, 1, 64) == AK_WIDE2 && attn_kernel_for(1, 0, 1, 384, 1, 64) == AK_NAIVE &&
              attn_kernel_for(2, 0, 1, 384, 1, 64) == AK_NAIVE && attn_kernel_for(2, 0, 1, 192, 1, 64) == AK_FLASH_F32, "D = 384 / 192 at 8 x 8");
static_assert(attn_kernel_for(0, 0, 1, 48, 1, 64) == AK_NAIVE && attn_kernel_for(0, 0, 1, 384, 1, 16) == AK_NAIVE && attn_kernel_for(0, 0, 1, 96, 1, 64) == AK_SPLIT3 &&
              attn_kernel_for(0, 0, 1, 1056, 1, 64) == AK_NAIVE && attn_kernel_for(4, 0, 0, 1024, 1, 64) == AK_WIDE3 && attn_kernel_for(0, 0, 0, 384, 1, 64) == AK_NAIVE,
              "what stays naive; the cap; no split arithmetic on offer");
static_assert(attn_kernel_for(0, 0, 1, 192, 1, 1024) == AK_FLASH_F32 && attn_kernel_for(0, 1, 1, 192, 1, 1024) == AK_WIDE2 && attn_kernel_for(4, 0, 1, 256, 1, 256) == AK_WIDE3 &&
              attn_kernel_for(4, 0, 1, 160, 1, 288) == AK_FLASH_F32 && attn_kernel_for(0, 0, 1, 288, 1, 1024) == AK_WIDE3 && attn_kernel_for(0, 0, 1, 128, 1, 1024) == AK_SPLIT3,
              "160 ... 256: three pieces wide up to 256 tokens, two pieces wide at every token count; above 256 wide whatever the token count");
}  // namespace attn_kernels_check

}  // namespace mcvd
