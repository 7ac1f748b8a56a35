// The convolution kernel variants, once: what each "shape id" is, what it needs, what it turns into when an arithmetic option is off and
// what a launch tries after it.  The ids are public (the context options conv_shape / conv_shape1, the committed tuning tables under
// profiles/, mcvd_last_conv_kernel / mcvd_model_op_kernel): a new variant gets a new number and one line here; numbers are never reused.
// Plain C++17, no HIP: the static_asserts at the end check the table in every build.  Which launches the Winograd families take is the second
// table of this file (kWinoRules / wino_admits, below the id table); which ids the autotuner offers a layer is conv_tuner.h.
#pragma once
#include <cstddef>
#include <initializer_list>

namespace mcvd {

enum ConvKernel : int {
    CK_AUTO = -1,                 // the dispatcher's own choice (kernels/conv.cpp)
    CK_TILE256 = 0, CK_TILE128 = 1, CK_TILE64 = 2, CK_TILE_SPLITK = 3,
    CK_WINO = 4, CK_DMA1 = 5, CK_DMA1_CK32 = 6, /* 7 unused */ CK_WINO_K2 = 8, CK_DMA1_PX64 = 9,
    CK_WINO3 = 10, CK_WINO3_K2 = 11, CK_WINO2H = 12, CK_WINO2H_K2 = 13, CK_GEMM1_F16X2 = 14, CK_GEMM1_BF16X3 = 15,
    CK_WINO3P = 16, CK_WINO3P_K2 = 17, CK_WINO3_K4 = 18, CK_WINO3_K8 = 19, CK_WINO3P_K4 = 20, /* 21 unused */
    CK_GEMM3_TAPS = 22, CK_GEMM3_IM2COL = 23, CK_WINO1H = 24, CK_WINO1H_K2 = 25,
    CK_WINO2H_K4 = 26, CK_WINO1H_K4 = 27,
    CK_RETIRED_SPADE_WINO = 36, CK_RETIRED_SPADE_WINO_K2 = 40      // round-5 tables: the per-layer fused SPADE loader, gone; read as CK_AUTO
};

// Ordered: within the Winograd families a larger value is the more specialised kernel (fallback lists only ever go down).
enum ConvFamily : int {
    CF_NONE,        // not a kernel (CK_AUTO, unused and unknown ids)
    CF_TILE,        // direct implicit GEMM on the fp32 MFMA; the id is the pixel tile (conv_mfma.h)
    CF_DMA1,        // all-DMA 1x1 GEMM, fp32 MFMA (conv1x1_dma.cpp)
    CF_SPLIT1,      // split-operand 1x1 GEMM on the fp16 / bf16 pipe (conv1x1_h2.cpp)
    CF_GEMM3,       // a 3x3 as a CF_SPLIT1 GEMM plus a copy / shift pass (conv_gemm_forms.cpp); launched by the model, not by the dispatcher
    CF_WINO,        // Winograd F(2x2,3x3), fp32 MFMA (conv_wino.cpp)
    CF_WINO2H,      // ... on the fp16 pipe, two-piece operands (conv_wino2h.cpp)
    CF_WINO3,       // ... on the bf16 pipe, three-piece operands (conv_wino3.cpp)
    CF_WINO3P,      // ... the same as persistent workgroups (conv_wino3p.cpp)
    CF_WINO1H       // ... on the fp16 pipe, ONE-piece operands: a draft arithmetic (conv_wino2h.cpp, NP = 1)
};

enum ConvWeights : int { CW_WP, CW_WPW, CW_WPH, CW_WPB };      // the ConvArgs weight image the kernel reads

struct ConvKernelDesc {
    int id;
    const char* name;
    ConvFamily family;
    int ks;                // kernel size served (0: 1 and 3)
    int pieces;            // operand pieces: 0 fp32, 1 fp16 (one rounding: 11 bits), 2 fp16, 3 bf16
    int kparts;            // K split: 0 none, else ConvArgs::ksplit
    bool own_cot;          // takes a cout tile of its own (ConvArgs::cot is not the direct kernel's)
    ConvWeights weights;
    int no_f16x2;          // the id it becomes when the option f16x2 is off or the input is raw
    int no_bf16x3;         // the id it becomes when the option bf16x3 is off
    int no_f16x1;          // the id it becomes when the option f16x1 is off or the input is raw (applied in front of no_bf16x3)
    int fallback[7];       // what a launch with this hint tries, in order, each only if usable; -1 ends the list, then the direct-tile heuristic
};

inline constexpr ConvKernelDesc kConvKernels[] = {
    //  id               name              family     ks pc kp own_cot weights  no_f16x2         no_bf16x3        no_f16x1         fallback
    {CK_TILE256,      "tile256",        CF_TILE,    0, 0, 0, false, CW_WP,  CK_TILE256,      CK_TILE256,      CK_TILE256,      {-1}},
    {CK_TILE128,      "tile128",        CF_TILE,    0, 0, 0, false, CW_WP,  CK_TILE128,      CK_TILE128,      CK_TILE128,      {-1}},
    {CK_TILE64,       "tile64",         CF_TILE,    0, 0, 0, false, CW_WP,  CK_TILE64,       CK_TILE64,       CK_TILE64,       {-1}},
    {CK_TILE_SPLITK,  "tile64_splitk",  CF_TILE,    0, 0, 0, false, CW_WP,  CK_TILE_SPLITK,  CK_TILE_SPLITK,  CK_TILE_SPLITK,  {-1}},
    {CK_WINO,         "wino",           CF_WINO,    3, 0, 0, false, CW_WPW, CK_WINO,         CK_WINO,         CK_WINO,         {CK_WINO, -1}},
    {CK_DMA1,         "dma1",           CF_DMA1,    1, 0, 0, true,  CW_WP,  CK_DMA1,         CK_DMA1,         CK_DMA1,         {CK_DMA1, -1}},
    {CK_DMA1_CK32,    "dma1_ck32",      CF_DMA1,    1, 0, 0, true,  CW_WP,  CK_DMA1_CK32,    CK_DMA1_CK32,    CK_DMA1_CK32,    {CK_DMA1_CK32, -1}},
    {CK_WINO_K2,      "wino_k2",        CF_WINO,    3, 0, 2, false, CW_WPW, CK_WINO_K2,      CK_WINO_K2,      CK_WINO_K2,      {CK_WINO_K2, CK_WINO, -1}},
    {CK_DMA1_PX64,    "dma1_px64",      CF_DMA1,    1, 0, 0, true,  CW_WP,  CK_DMA1_PX64,    CK_DMA1_PX64,    CK_DMA1_PX64,    {CK_DMA1_PX64, -1}},
    {CK_WINO3,        "wino3",          CF_WINO3,   3, 3, 0, false, CW_WPB, CK_WINO3,        CK_WINO,         CK_WINO3,        {CK_WINO3, CK_WINO, -1}},
    {CK_WINO3_K2,     "wino3_k2",       CF_WINO3,   3, 3, 2, false, CW_WPB, CK_WINO3_K2,     CK_WINO_K2,      CK_WINO3_K2,     {CK_WINO3_K2, CK_WINO3, CK_WINO, -1}},
    {CK_WINO2H,       "wino2h",         CF_WINO2H,  3, 2, 0, false, CW_WPH, CK_WINO3,        CK_WINO2H,       CK_WINO2H,       {CK_WINO2H, CK_WINO, -1}},
    {CK_WINO2H_K2,    "wino2h_k2",      CF_WINO2H,  3, 2, 2, false, CW_WPH, CK_WINO3_K2,     CK_WINO2H_K2,    CK_WINO2H_K2,    {CK_WINO2H_K2, CK_WINO2H, CK_WINO, -1}},
    {CK_GEMM1_F16X2,  "gemm1_f16x2",    CF_SPLIT1,  1, 2, 0, true,  CW_WPH, CK_GEMM1_BF16X3, CK_GEMM1_F16X2,  CK_GEMM1_F16X2,  {CK_GEMM1_F16X2, -1}},
    {CK_GEMM1_BF16X3, "gemm1_bf16x3",   CF_SPLIT1,  1, 3, 0, true,  CW_WPB, CK_GEMM1_BF16X3, CK_DMA1,         CK_GEMM1_BF16X3, {CK_GEMM1_BF16X3, -1}},
    {CK_WINO3P,       "wino3p",         CF_WINO3P,  3, 3, 0, false, CW_WPB, CK_WINO3P,       CK_WINO,         CK_WINO3P,       {CK_WINO3P, CK_WINO3, CK_WINO, -1}},
    {CK_WINO3P_K2,    "wino3p_k2",      CF_WINO3P,  3, 3, 2, false, CW_WPB, CK_WINO3P_K2,    CK_WINO_K2,      CK_WINO3P_K2,    {CK_WINO3P_K2, CK_WINO3P, CK_WINO3_K2, CK_WINO3, CK_WINO, -1}},
    {CK_WINO3_K4,     "wino3_k4",       CF_WINO3,   3, 3, 4, false, CW_WPB, CK_WINO3_K4,     CK_WINO_K2,      CK_WINO3_K4,     {CK_WINO3_K4, CK_WINO3_K2, CK_WINO3, CK_WINO, -1}},
    {CK_WINO3_K8,     "wino3_k8",       CF_WINO3,   3, 3, 8, false, CW_WPB, CK_WINO3_K8,     CK_WINO_K2,      CK_WINO3_K8,     {CK_WINO3_K8, CK_WINO3_K4, CK_WINO3_K2, CK_WINO3, CK_WINO, -1}},
    {CK_WINO3P_K4,    "wino3p_k4",      CF_WINO3P,  3, 3, 4, false, CW_WPB, CK_WINO3P_K4,    CK_WINO_K2,      CK_WINO3P_K4,    {CK_WINO3P_K4, CK_WINO3P_K2, CK_WINO3P, CK_WINO3_K2, CK_WINO3, CK_WINO, -1}},
    {CK_GEMM3_TAPS,   "gemm3_taps",     CF_GEMM3,   3, 3, 0, true,  CW_WPB, CK_GEMM3_TAPS,   CK_GEMM3_TAPS,   CK_GEMM3_TAPS,   {-1}},     // (bf16x3 off: the model falls
    {CK_GEMM3_IM2COL, "gemm3_im2col",   CF_GEMM3,   3, 3, 0, true,  CW_WPB, CK_GEMM3_IM2COL, CK_GEMM3_IM2COL, CK_GEMM3_IM2COL, {-1}},     //  back to CK_AUTO itself)
    {CK_WINO1H,       "wino1h",         CF_WINO1H,  3, 1, 0, false, CW_WPH, CK_WINO1H,       CK_WINO1H,       CK_WINO3,        {CK_WINO1H, CK_WINO, -1}},
    {CK_WINO1H_K2,    "wino1h_k2",      CF_WINO1H,  3, 1, 2, false, CW_WPH, CK_WINO1H_K2,    CK_WINO1H_K2,    CK_WINO3_K2,     {CK_WINO1H_K2, CK_WINO1H, CK_WINO, -1}},
    {CK_WINO2H_K4,    "wino2h_k4",      CF_WINO2H,  3, 2, 4, false, CW_WPH, CK_WINO3_K4,     CK_WINO2H_K4,    CK_WINO2H_K4,    {CK_WINO2H_K4, CK_WINO2H_K2, CK_WINO2H, CK_WINO, -1}},
    {CK_WINO1H_K4,    "wino1h_k4",      CF_WINO1H,  3, 1, 4, false, CW_WPH, CK_WINO1H_K4,    CK_WINO1H_K4,    CK_WINO3_K4,     {CK_WINO1H_K4, CK_WINO1H_K2, CK_WINO1H, CK_WINO, -1}},
};
inline constexpr ConvKernelDesc kNoConvKernel = {CK_AUTO, "auto", CF_NONE, 0, 0, 0, false, CW_WP, CK_AUTO, CK_AUTO, CK_AUTO, {-1}};

// the descriptor of an id; kNoConvKernel for CK_AUTO and for anything that is not a kernel (an option or an imported table can hold any integer)
constexpr const ConvKernelDesc& conv_kernel(int id) {
    for (const ConvKernelDesc& k : kConvKernels)
        if (k.id == id) return k;
    return kNoConvKernel;
}
constexpr bool is_winograd(int id) { return conv_kernel(id).family >= CF_WINO; }
constexpr int k_parts(int id) { return conv_kernel(id).kparts; }
constexpr int pieces(int id) { return conv_kernel(id).pieces; }
constexpr int without_f16x2(int id) { return conv_kernel(id).id == id ? conv_kernel(id).no_f16x2 : id; }
constexpr int without_bf16x3(int id) { return conv_kernel(id).id == id ? conv_kernel(id).no_bf16x3 : id; }
constexpr int without_f16x1(int id) { return conv_kernel(id).id == id ? conv_kernel(id).no_f16x1 : id; }

// ---- which launches the Winograd families take ----
// A workgroup parks the GroupNorm (A, B) coefficients of the channels ITS 16-channel chunks contract -- all of them without a K split, one
// part's with one -- in an LDS table.  A workgroup of 8 x 16-pixel regions (every plane but 8 x 8) serves ONE sample and parks up to
// WINO_TABLE_CH_PLANE entries (four per thread of the 512-thread kernels, two per thread of conv_wino.cpp's 1024); an 8 x 8 launch serves TWO
// samples per workgroup and parks up to WINO_TABLE_CH entries for each: four entries for two samples do not fit the LDS.  So a launch needs
//     Cin <= wino_max_cin(parts)   and   CinP / parts <= wino_table_ch(8 x 8 ?):
// on planes of 16 x 16 and larger the unsplit ids 4 / 10 / 12 / 24 take every layer up to 2048 channels -- no K-split scratch, so also the
// 32 x 32 layers of a model above 1024 channels; at 8 x 8 they stop at 1024 and layers of 1040 .. 2048 channels are served by the K-split ids
// 8 / 11 / 18 / 19 / 13 / 26 / 25 / 27 where the split's own conditions hold.  A split of four or more parts takes WINO_MAX_CIN_K4 channels (144
// chunks: 576 per part at 4 parts, 288 at 8): layers of 2049 .. 2304 (the concats of the ngf-288 UCF-101 nets) are served by ids 18 / 19
// (bf16x3), 26 (f16x2) and 27 (f16x1) only.  The 2-way and unsplit launches stop at WINO_MAX_CIN -- the 2-way split by this constant alone
// on a plane, where a part of 1152 channels would fit the table: its part buffers and the tuner's candidate rules are sized for it -- and
// CF_WINO has no 4-way split: with bf16x3 off such a layer runs the direct tile kernel.
// The persistent kernel (CF_WINO3P) was NOT widened: it keeps one table of ALL Cin channels per run of items of a sample, split or not (an
// item of another part would need its table reloaded inside the item boundary), so it stops at WINO_TABLE_CH; its fallback lists
// (17 -> 11, 20 -> 17 -> 16 -> 11) route round it.  The SPADE-fused loader of CF_WINO (ConvArgs::gb) stays at WINO_TABLE_CH as well.
// The LDS request is no term of the rule: each kernel file static_asserts that the widest table its row admits fits a CU's 160 KiB.
constexpr int WINO_MAX_CIN = 2048;
constexpr int WINO_MAX_CIN_K4 = 2304;          // a split of four or more parts takes this many
constexpr int WINO_TABLE_CH = 1024;            // table entries per sample, 8 x 8 launches (two samples per workgroup); the persistent kernel; the SPADE-fused loader
constexpr int WINO_TABLE_CH_PLANE = 2048;      // ... launches of 8 x 16-pixel regions (one sample per workgroup)
static_assert(WINO_TABLE_CH_PLANE == 2 * WINO_TABLE_CH && WINO_MAX_CIN <= WINO_TABLE_CH_PLANE, "an unsplit plane launch parks every channel up to WINO_MAX_CIN");
static_assert(WINO_MAX_CIN_K4 > 2 * WINO_TABLE_CH && WINO_MAX_CIN <= 2 * WINO_TABLE_CH, "above WINO_MAX_CIN a 2-way part overflows the 8 x 8 table");
constexpr int wino_max_cin(int parts) { return parts >= 4 ? WINO_MAX_CIN_K4 : WINO_MAX_CIN; }
constexpr int wino_table_ch(bool g8) { return g8 ? WINO_TABLE_CH : WINO_TABLE_CH_PLANE; }
constexpr int wino_part_channels(int CinP, int parts) { return CinP / (parts >= 2 ? parts : 1); }      // PC: the table's entries per sample
// the K parts a kernel makes of ConvArgs::ksplit.  conv_wino.cpp counts 2 as a split and every other value, 4 included, as none; the others
// take the value as it comes, and the rule refuses the counts their row does not have
constexpr int wino_kernel_parts(ConvFamily f, int ksplit) { return f == CF_WINO ? (ksplit == 2 ? 2 : 1) : ksplit; }

struct WinoLaunch {        // what the rule reads of a launch
    int ks, H, W, B, Cin, CinP, C0, C1, Cout, CoutP;
    int parts;             // wino_kernel_parts(family, ConvArgs::ksplit)
    bool weights;          // the family's weight image is present
    bool spade;            // ConvArgs::gb: the SPADE-fused loader
    size_t part_floats;    // room for the K split's partial results, in floats; 0: no scratch
};

struct WinoRule {
    ConvFamily family;
    int chunk;             // input channels per chunk: CinP is a multiple, and no chunk straddles the concat seam
    bool g8;               // serves 8 x 8 images in pairs, next to regions of 8 x 16 pixels
    int max_hw;            // H * W at most; 0: no cap
    int min_chunks[4];     // fewest chunks per part of an unsplit launch and of 2, 4, 8 parts; 0: the family has no such split
    bool spade;            // has the SPADE-fused loader, for Cin <= WINO_TABLE_CH
    bool persistent;       // one table of all Cin channels (Cin <= WINO_TABLE_CH, split or not); 32-bit item count
};
inline constexpr WinoRule kWinoRules[] = {
    // family    chunk  g8    max_hw  min_chunks      spade  persistent
    {CF_WINO,     16,  true,  0,      {1, 2, 0, 0},   true,  false},
    {CF_WINO2H,   16,  true,  16384,  {1, 2, 3, 0},   false, false},     // CF_WINO1H as well: one rule for both piece counts; 4 parts: the prologue requests three chunks
    {CF_WINO3,    16,  true,  16384,  {1, 2, 2, 2},   false, false},
    {CF_WINO3P,   16,  false, 16384,  {4, 4, 4, 4},   false, true},      // the stream of an item needs four chunks
};
constexpr const WinoRule* wino_rule(ConvFamily f) {
    for (const WinoRule& r : kWinoRules)
        if (r.family == (f == CF_WINO1H ? CF_WINO2H : f)) return &r;
    return nullptr;
}

constexpr bool wino_admits(ConvFamily f, const WinoLaunch& l) {
    const WinoRule* r = wino_rule(f);
    if (!r || l.ks != 3 || !l.weights) return false;
    const bool g8 = l.H == 8 && l.W == 8;
    if (!((l.H % 8 == 0 && l.W % 16 == 0 && l.H >= 8 && l.W >= 16) || (r->g8 && g8))) return false;
    if (r->max_hw && l.H * l.W > r->max_hw) return false;
    if (l.CinP % r->chunk != 0 || (l.C1 != 0 && l.C0 % r->chunk != 0)) return false;
    if ((long)l.B * (l.C0 > l.C1 ? l.C0 : l.C1) * l.H * l.W >= (1L << 29)) return false;      // 32-bit byte offsets of the patch loads
    if (l.spade && !(r->spade && l.Cin <= WINO_TABLE_CH)) return false;
    const int parts = l.parts >= 2 ? l.parts : 1;
    const int slot = parts == 1 ? 0 : parts == 2 ? 1 : parts == 4 ? 2 : parts == 8 ? 3 : -1;
    if (slot < 0 || r->min_chunks[slot] == 0) return false;
    const int nch = l.CinP / r->chunk;
    if (nch % parts != 0 || nch / parts < r->min_chunks[slot]) return false;
    if (r->persistent) {
        if (l.Cin > WINO_TABLE_CH || (long)l.B * (l.H / 8) * (l.W / 16) * (l.CoutP / 32) * 8 >= (1L << 31)) return false;
    } else if (l.Cin > wino_max_cin(parts) || wino_part_channels(l.CinP, parts) > wino_table_ch(g8)) {
        return false;
    }
    return parts == 1 || (l.part_floats != 0 && (size_t)parts * l.B * l.Cout * l.H * l.W <= l.part_floats);
}

// ---- the table, checked ----
namespace conv_kernels_check {
constexpr int N = sizeof(kConvKernels) / sizeof(kConvKernels[0]);
constexpr bool known(int id) { return conv_kernel(id).id == id && id != CK_AUTO; }
constexpr int rank(const ConvKernelDesc& k) { return k.family * 16 + k.kparts; }       // "simpler" = lower
constexpr bool fallback_is(int id, std::initializer_list<int> want) {
    const int* f = conv_kernel(id).fallback;
    for (int w : want)
        if (*f++ != w) return false;
    return *f == -1;
}
constexpr bool ids_unique() {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < i; ++j)
            if (kConvKernels[i].id == kConvKernels[j].id) return false;
    return true;
}
// a list is empty or starts with its own id, names kernels of the same size only, gets strictly simpler and, for a Winograd id, ends in CK_WINO
constexpr bool fallbacks_sound() {
    for (const ConvKernelDesc& k : kConvKernels) {
        const ConvKernelDesc* prev = nullptr;
        for (const int* f = k.fallback; *f != -1; ++f) {
            const ConvKernelDesc& e = conv_kernel(*f);
            if (!known(*f) || e.ks != k.ks || (prev ? rank(e) >= rank(*prev) : e.id != k.id)) return false;
            prev = &e;
        }
        if (k.family >= CF_WINO ? (!prev || prev->id != CK_WINO) : (prev && prev->id != k.id)) return false;
        if ((k.family == CF_TILE || k.family == CF_GEMM3) && prev) return false;
    }
    return true;
}
// a remap stays within the kernel size, drops exactly the pieces the option names and keeps a K split where the target family has one
constexpr bool remaps_sound() {
    for (const ConvKernelDesc& k : kConvKernels) {
        const ConvKernelDesc &f = conv_kernel(k.no_f16x2), &b = conv_kernel(k.no_bf16x3), &o = conv_kernel(k.no_f16x1);
        if (!known(k.no_f16x2) || !known(k.no_bf16x3) || !known(k.no_f16x1) || f.ks != k.ks || b.ks != k.ks || o.ks != k.ks) return false;
        if (k.pieces == 1 ? (o.pieces != 3 || o.kparts != k.kparts) : o.id != k.id) return false;
        if (k.pieces == 2 ? (f.pieces != 3 || f.kparts != k.kparts) : f.id != k.id) return false;
        if (k.pieces == 3 && k.family != CF_GEMM3 ? (b.pieces != 0 || (b.kparts != 0) != (k.kparts != 0)) : b.id != k.id) return false;
    }
    return true;
}
static_assert(ids_unique(), "conv kernel ids must be unique");
static_assert(!known(7) && !known(21) && !known(CK_AUTO) && !known(CK_RETIRED_SPADE_WINO) && !known(CK_RETIRED_SPADE_WINO_K2), "7 and 21 stay unused; retired ids are not kernels");
static_assert(fallbacks_sound(), "a fallback list names an unknown id, another kernel size, or does not get simpler");
static_assert(remaps_sound(), "an option remap names an unknown id, changes the kernel size, drops the wrong pieces or loses the K split");
static_assert(fallback_is(CK_WINO1H_K4, {27, 25, 24, 4}), "fallback list of 27");
static_assert(fallback_is(CK_WINO2H_K4, {26, 13, 12, 4}), "fallback list of 26");
static_assert(fallback_is(CK_WINO1H_K2, {25, 24, 4}), "fallback list of 25");
static_assert(fallback_is(CK_WINO1H, {24, 4}), "fallback list of 24");
static_assert(fallback_is(CK_WINO3P_K4, {20, 17, 16, 11, 10, 4}), "fallback list of 20");
static_assert(fallback_is(CK_WINO3_K8, {19, 18, 11, 10, 4}), "fallback list of 19");
static_assert(fallback_is(CK_WINO3_K4, {18, 11, 10, 4}), "fallback list of 18");
static_assert(fallback_is(CK_WINO3P_K2, {17, 16, 11, 10, 4}), "fallback list of 17");
static_assert(fallback_is(CK_WINO3P, {16, 10, 4}), "fallback list of 16");
static_assert(fallback_is(CK_WINO2H_K2, {13, 12, 4}), "fallback list of 13");
static_assert(fallback_is(CK_WINO2H, {12, 4}), "fallback list of 12");
static_assert(fallback_is(CK_WINO3_K2, {11, 10, 4}), "fallback list of 11");
static_assert(fallback_is(CK_WINO3, {10, 4}), "fallback list of 10");
static_assert(fallback_is(CK_WINO_K2, {8, 4}), "fallback list of 8");
static_assert(fallback_is(CK_WINO, {4}), "fallback list of 4");
static_assert(fallback_is(15, {15}) && fallback_is(14, {14}) && fallback_is(5, {5}) && fallback_is(6, {6}) && fallback_is(9, {9}), "the 1x1 GEMMs try themselves only");
static_assert(fallback_is(0, {}) && fallback_is(3, {}) && fallback_is(22, {}) && fallback_is(23, {}) && fallback_is(7, {}) && fallback_is(CK_AUTO, {}), "everything else: the tile heuristic");
static_assert(without_f16x2(12) == 10 && without_f16x2(13) == 11 && without_f16x2(14) == 15 && without_f16x2(15) == 15 && without_f16x2(99) == 99, "f16x2 off");
static_assert(without_bf16x3(10) == 4 && without_bf16x3(16) == 4 && without_bf16x3(15) == 5 && without_bf16x3(11) == 8 && without_bf16x3(17) == 8 &&
              without_bf16x3(18) == 8 && without_bf16x3(19) == 8 && without_bf16x3(20) == 8 && without_bf16x3(22) == 22 && without_bf16x3(99) == 99, "bf16x3 off");
static_assert(without_f16x1(24) == 10 && without_f16x1(25) == 11 && without_f16x1(12) == 12 && without_f16x1(10) == 10 && without_f16x1(99) == 99 &&
              without_f16x2(24) == 24 && without_bf16x3(25) == 25, "f16x1 off: the one-piece ids become the three-piece ones; the other options leave them alone");
static_assert(without_bf16x3(without_f16x1(24)) == 4 && without_bf16x3(without_f16x1(25)) == 8, "f16x1 and bf16x3 off: the fp32-MFMA kernels");
static_assert(pieces(24) == 1 && pieces(25) == 1 && k_parts(25) == 2 && is_winograd(24) && is_winograd(25), "the one-piece rows");
static_assert(CK_WINO2H_K4 == 26 && CK_WINO1H_K4 == 27 && pieces(26) == 2 && pieces(27) == 1 && k_parts(26) == 4 && k_parts(27) == 4 &&
              conv_kernel(26).family == CF_WINO2H && conv_kernel(27).family == CF_WINO1H, "the 4-way K split of the two fp16 Winograd kernels");
static_assert(without_f16x2(26) == 18 && without_f16x1(26) == 26 && without_bf16x3(26) == 26 && without_f16x1(27) == 18 && without_f16x2(27) == 27 &&
              without_bf16x3(27) == 27, "their option off: the three-piece 4-way split; the other options leave them alone");
static_assert(without_bf16x3(without_f16x2(26)) == 8 && without_bf16x3(without_f16x1(27)) == 8, "... and bf16x3 off as well: the fp32-MFMA 2-way split");

// the admission rule over concrete launches: B = 2, Cout = 32, a square plane, weights present, room for exactly the parts.  ksplit is
// ConvArgs::ksplit as a caller hands it over; C0 = 0: one source.  tests/test_wino_rule_cpu.py evaluates the same list with tests/wino_rule.py.
struct WinoCase { ConvFamily family; int Cin, CinP, ksplit, plane, C0; bool spade, admitted; };
inline constexpr WinoCase kWinoCases[] = {
    // the two table sizes: 1024 entries per sample at 8 x 8, 2048 on a plane
    {CF_WINO3, 1040, 1040, 0, 8, 0, false, false},  {CF_WINO3, 1040, 1040, 0, 16, 0, false, true},
    {CF_WINO3, 1024, 1024, 0, 8, 0, false, true},   {CF_WINO3, 1024, 1024, 0, 16, 0, false, true},
    {CF_WINO3, 2048, 2048, 0, 16, 0, false, true},  {CF_WINO3, 2035, 2048, 0, 16, 0, false, true},   {CF_WINO3, 2048, 2048, 0, 8, 0, false, false},
    {CF_WINO3, 2064, 2064, 0, 8, 0, false, false},  {CF_WINO3, 2064, 2064, 0, 16, 0, false, false},
    {CF_WINO3, 2049, 2064, 0, 8, 0, false, false},  {CF_WINO3, 2049, 2064, 0, 16, 0, false, false},
    {CF_WINO3, 1440, 1440, 0, 32, 0, false, true},  {CF_WINO3, 1152, 1152, 0, 32, 0, false, true},
    {CF_WINO3, 1344, 1344, 0, 16, 0, false, true},  {CF_WINO3, 1728, 1728, 0, 16, 0, false, true},
    // 2304 channels: four parts or eight; two parts are refused by the channel bound even where a part of 1152 channels fits the table
    {CF_WINO3, 2304, 2304, 2, 8, 0, false, false},  {CF_WINO3, 2304, 2304, 2, 16, 0, false, false},  {CF_WINO3, 2304, 2304, 0, 16, 0, false, false},
    {CF_WINO3, 2304, 2304, 4, 8, 0, false, true},   {CF_WINO3, 2304, 2304, 4, 16, 0, false, true},   {CF_WINO3, 2304, 2304, 8, 8, 0, false, true},
    {CF_WINO3, 2290, 2304, 4, 8, 0, false, true},   {CF_WINO3, 2320, 2320, 4, 8, 0, false, false},   {CF_WINO3, 2160, 2160, 4, 8, 0, false, false},
    {CF_WINO2H, 2304, 2304, 4, 8, 0, false, true},  {CF_WINO1H, 2304, 2304, 4, 16, 0, false, true},  {CF_WINO2H, 2304, 2304, 2, 16, 0, false, false},
    // part counts a family does not have
    {CF_WINO2H, 2304, 2304, 8, 8, 0, false, false}, {CF_WINO3, 768, 768, 3, 8, 0, false, false},     {CF_WINO3, 1024, 1024, 16, 8, 0, false, false},
    {CF_WINO3P, 768, 768, 16, 16, 0, false, false}, {CF_WINO1H, 768, 768, 3, 16, 0, false, false},
    // the 4-way split of the fp16 kernels: chunks that divide by 4, three per part at least, no chunk across the seam
    {CF_WINO2H, 192, 192, 4, 8, 0, false, true},    {CF_WINO2H, 128, 128, 4, 8, 0, false, false},    {CF_WINO2H, 288, 288, 4, 8, 0, false, false},
    {CF_WINO2H, 256, 256, 4, 8, 100, false, false}, {CF_WINO2H, 256, 256, 4, 8, 160, false, true},   {CF_WINO2H, 250, 256, 4, 8, 0, false, true},
    {CF_WINO2H, 1088, 1088, 4, 8, 0, false, true},  {CF_WINO2H, 1040, 1040, 4, 8, 0, false, false},  {CF_WINO2H, 2320, 2320, 4, 8, 0, false, false},
    {CF_WINO1H, 192, 192, 4, 16, 0, false, true},   {CF_WINO1H, 128, 128, 4, 16, 0, false, false},   {CF_WINO3, 128, 128, 4, 16, 0, false, true},
    // the persistent kernel: all of Cin in one table, four chunks per part, regions only
    {CF_WINO3P, 1040, 1040, 0, 16, 0, false, false}, {CF_WINO3P, 1040, 1040, 2, 16, 0, false, false}, {CF_WINO3P, 1024, 1024, 2, 16, 0, false, true},
    {CF_WINO3P, 48, 48, 0, 16, 0, false, false},    {CF_WINO3P, 96, 96, 2, 16, 0, false, false},     {CF_WINO3P, 96, 96, 0, 16, 0, false, true},
    {CF_WINO3P, 256, 256, 0, 8, 0, false, false},   {CF_WINO3, 256, 256, 0, 8, 0, false, true},
    // conv_wino.cpp: the SPADE-fused loader stays at 1024 channels; only 2 is a split
    {CF_WINO, 1152, 1152, 0, 16, 0, true, false},   {CF_WINO, 1152, 1152, 0, 16, 0, false, true},    {CF_WINO, 1024, 1024, 0, 16, 0, true, true},
    {CF_WINO3, 256, 256, 0, 16, 0, true, false},    {CF_WINO, 48, 48, 2, 8, 0, false, false},        {CF_WINO, 48, 48, 4, 8, 0, false, true},
    {CF_WINO, 1152, 1152, 4, 8, 0, false, false},   {CF_WINO, 1152, 1152, 2, 8, 0, false, true},     {CF_WINO, 2304, 2304, 2, 16, 0, false, false},
};
constexpr WinoLaunch wino_case_launch(const WinoCase& c) {
    const int parts = wino_kernel_parts(c.family, c.ksplit);
    return {3, c.plane, c.plane, 2, c.Cin, c.CinP, c.C0 ? c.C0 : c.Cin, c.C0 ? c.Cin - c.C0 : 0, 32, 32, parts, true, c.spade,
            parts >= 2 ? (size_t)parts * 2 * 32 * c.plane * c.plane : 0};
}
constexpr int first_wrong_wino_case() {
    int i = 0;
    for (const WinoCase& c : kWinoCases) {
        if (wino_admits(c.family, wino_case_launch(c)) != c.admitted) return i;
        ++i;
    }
    return -1;
}
static_assert(first_wrong_wino_case() == -1, "the admission rule disagrees with kWinoCases at this index");
constexpr WinoLaunch with_room(WinoLaunch l, size_t part_floats) { l.part_floats = part_floats; return l; }
static_assert(!wino_admits(CF_WINO3, with_room(wino_case_launch({CF_WINO3, 1056, 1056, 2, 8, 0, false, true}), 2 * 2 * 32 * 64 - 1)) &&
              !wino_admits(CF_WINO3, with_room(wino_case_launch({CF_WINO3, 1056, 1056, 2, 8, 0, false, true}), 0)) &&
              wino_admits(CF_WINO3, with_room(wino_case_launch({CF_WINO3, 1056, 1056, 2, 8, 0, false, true}), 2 * 2 * 32 * 64)),
              "a K split needs room for its partial results");

// the rule's geometric clause over planes that are not square: B = 2, Cout = 32, one source, CinP = Cin, weights present, room for exactly the
// parts.  `parts` is what the kernel makes of the split (wino_kernel_parts), not ConvArgs::ksplit.  tests/test_wino_rule_cpu.py evaluates the
// same list with tests/wino_rule.py; tests/test_gpu_conv_paths.py runs the admitted shapes and the refusals on the device.
struct WinoPlaneCase { ConvFamily family; int H, W, parts, Cin; bool admitted; };
inline constexpr WinoPlaneCase kWinoPlaneCases[] = {
    // regions of 8 x 16 pixels: H a multiple of 8 (a power of two or not), W a multiple of 16
    {CF_WINO3, 8, 16, 1, 64, true},      {CF_WINO3, 16, 32, 1, 64, true},     {CF_WINO3, 32, 16, 1, 64, true},    {CF_WINO3, 24, 16, 1, 64, true},
    {CF_WINO3, 8, 32, 1, 64, true},      {CF_WINO3P, 8, 16, 1, 64, true},     {CF_WINO, 24, 16, 1, 64, true},     {CF_WINO1H, 8, 32, 1, 64, true},
    {CF_WINO3, 16, 8, 1, 64, false},     {CF_WINO, 16, 8, 1, 64, false},      {CF_WINO3, 8, 24, 1, 64, false},    {CF_WINO3, 4, 16, 1, 64, false},
    {CF_WINO3, 12, 16, 1, 64, false},    {CF_WINO2H, 12, 16, 1, 64, false},   {CF_WINO3P, 12, 16, 1, 64, false},  {CF_WINO, 12, 16, 1, 64, false},
    // 8 x 8: pairs of images, every family but the persistent one
    {CF_WINO, 8, 8, 1, 64, true},        {CF_WINO2H, 8, 8, 1, 64, true},      {CF_WINO1H, 8, 8, 1, 64, true},     {CF_WINO3, 8, 8, 1, 64, true},
    {CF_WINO3P, 8, 8, 1, 64, false},
    // max_hw: 16384 pixels but for conv_wino.cpp
    {CF_WINO3, 128, 128, 1, 64, true},   {CF_WINO3, 128, 256, 1, 64, false},  {CF_WINO2H, 128, 256, 1, 64, false}, {CF_WINO3P, 128, 256, 1, 64, false},
    {CF_WINO, 128, 256, 1, 64, true},    {CF_WINO3, 64, 256, 1, 64, true},
    // a split on one region and on a plane whose H is no power of two
    {CF_WINO3, 8, 16, 2, 64, true},      {CF_WINO3, 8, 16, 4, 64, false},     {CF_WINO2H, 24, 16, 4, 192, true},  {CF_WINO3P, 24, 16, 2, 128, true},
    {CF_WINO, 8, 32, 2, 64, true},
};
constexpr WinoLaunch wino_plane_case_launch(const WinoPlaneCase& c) {
    return {3, c.H, c.W, 2, c.Cin, c.Cin, c.Cin, 0, 32, 32, c.parts, true, false, c.parts >= 2 ? (size_t)c.parts * 2 * 32 * c.H * c.W : 0};
}
constexpr int first_wrong_wino_plane_case() {
    int i = 0;
    for (const WinoPlaneCase& c : kWinoPlaneCases) {
        if (wino_admits(c.family, wino_plane_case_launch(c)) != c.admitted) return i;
        ++i;
    }
    return -1;
}
static_assert(first_wrong_wino_plane_case() == -1, "the admission rule disagrees with kWinoPlaneCases at this index");
}  // namespace conv_kernels_check

}  // namespace mcvd
