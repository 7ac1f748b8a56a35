// The conv autotuner's candidate rule, once: which kernel ids (conv_kernels.h) mcvd_model::autotune times for which layer under which options,
// and in which order -- the tuner keeps a candidate only on a strictly smaller time, so the order is part of the behaviour.
// mcvd_model::ensure_ksplit sizes the K-split scratch from the same rule (tuner_deepest_split): what the tuner can time always fits.
// Plain C++17, no HIP and no pointers: the static_asserts at the end check the rule in every build.
#pragma once
#include <initializer_list>

#include "conv_kernels.h"

namespace mcvd {

struct TunerLayer {        // what the rule reads of a conv op at a batch size
    int ks, H, W, B, Cin, Cout, CoutP;
    int cot;               // the op's own cout tile (conv_cout_tile)
    int wino_cot;          // the Winograd kernels' cout tile (conv_wino_cout_tile)
    bool raw;              // no norm in front of the conv (conv_input_raw): the fp16 arithmetics stay away
    bool spade;            // a SPADE norm in front of the conv
    int alt_kind;          // the GEMM form of a 3x3 (CK_GEMM3_TAPS / CK_GEMM3_IM2COL), 0: none
};

struct TunerOptions {      // the context options the rule reads: a table tuned under another signature is dropped (sync_tuning_options)
    bool winograd, conv_dma1, bf16x3, f16x2, f16x1, spade_fuse, conv_wdma;
    constexpr int signature() const {
        return (winograd ? 1 : 0) | (conv_dma1 ? 2 : 0) | (bf16x3 ? 4 : 0) | (f16x2 ? 8 : 0) | (spade_fuse ? 16 : 0) | (conv_wdma ? 32 : 0) | (f16x1 ? 64 : 0);
    }
};

// (region, cout tile) pairs of a Winograd launch (8 x 8 planes go in pairs of samples): few of them leave CUs idle, and the deeper K splits
// are offered -- 4 parts where the 2-way split leaves the chip with less than a few workgroups per CU, 8 where the 4-way one does (the
// measurement decides; above that the reduce pass only costs)
constexpr long tuner_pairs(const TunerLayer& l) {
    if (l.ks != 3) return 0;
    const bool g8 = l.H == 8 && l.W == 8;
    return (g8 ? (l.B + 1) / 2 : (long)l.B * (l.H / 8) * (l.W / 16)) * (l.CoutP / (32 * l.wino_cot));
}
// a layer of more than WINO_MAX_CIN channels has no 2-way split to fall back on -- 4 parts are the shallowest Winograd launch that takes it --
// so it is offered the 4-way ids at every batch; the 8-way one on the terms of every other layer
constexpr bool wino_needs_4_parts(int Cin) { return Cin > WINO_MAX_CIN; }
constexpr bool tuner_few_pairs(const TunerLayer& l) { return l.ks == 3 && (2 * tuner_pairs(l) < 1024 || wino_needs_4_parts(l.Cin)); }

// The ordered (id, cout tile) candidates of a layer.  usable(id, cot): the kernel takes the layer's real launch with this cout tile
// (conv_kernel_usable; gemm_form_usable for the GEMM forms, of which the caller also skips the tiles gemm_form_args would change).  The direct
// tiles are never asked.  emit(id, cot) times one candidate; a non-zero return ends the enumeration and is returned.
//
// f16x2 / f16x1 range guard: the fp16 kernels see NORMALISED inputs only -- GroupNorm-ed (O(1) by construction) or SPADE-normalised, which is
// the tensor spade_apply materialises (as bounded as the other up to the cond-derived gamma / beta: an overflow there ends as NaN in eps, which
// the non-finite scan reports as MCVD_ERANGE).  A conv over a RAW tensor (stem, shortcuts, NIN_3, the SPADE prep convs) has no bound on its
// input and stays on the fp32-range kernels.  With spade_fuse = 1 the modulation stays in the fp32 Winograd loader: no other kernel has it.
template <class Usable, class Emit>
constexpr int tuner_candidates(const TunerLayer& l, const TunerOptions& o, Usable&& usable, Emit&& emit) {
    auto offer = [&](bool when, std::initializer_list<int> ids, int cot) -> int {      // each id where the clause holds and the kernel takes the layer
        if (!when) return 0;
        for (int id : ids)
            if (usable(id, cot))
                if (int rc = emit(id, cot)) return rc;
        return 0;
    };
    const bool wino3 = l.ks == 3 && o.winograd, wino = wino3 && usable(CK_WINO, l.cot);
    const bool fused = l.spade && o.spade_fuse && o.winograd;      // the SPADE modulation runs in the conv's loader: the fp32 Winograd kernel only
    const bool few = tuner_few_pairs(l), fewer = few && 4 * tuner_pairs(l) < 1024;
    // the direct tiles (a tile of 256 / 128 / 64 pixels covers whole rows of the plane, or whole planes; 3: split-K with double-buffered
    // weights) and the fp32 Winograd kernel at the op's cout tile; the tiles again at cout tile 1
    for (int pass = 0; pass < (l.cot == 1 ? 1 : 2); ++pass)
        for (int id = CK_TILE256; id <= CK_WINO; ++id) {
            const int bpx = id == CK_TILE256 ? 256 : id == CK_TILE128 ? 128 : 64;
            const bool fits = bpx % l.W == 0 && (bpx / l.W <= l.H ? l.H % (bpx / l.W) == 0 : (bpx / l.W) % l.H == 0);
            const bool splitk_ok = id != CK_TILE_SPLITK || (l.ks == 3 && o.conv_wdma);
            const bool offered = id == CK_WINO ? (pass == 0 && wino) : (fits && splitk_ok && !(fused && wino));
            if (offered)
                if (int rc = emit(id, pass == 0 ? l.cot : 1)) return rc;
        }
    for (int c = 4; c >= 1 && l.alt_kind && !l.spade && usable(l.alt_kind, c); --c)      // the conv as a 1x1 GEMM on the three-piece kernel + its copy / shift pass
        if (int rc = emit(l.alt_kind, c)) return rc;
    if (int rc = offer(wino3, {CK_WINO_K2}, l.cot)) return rc;                            // the K split fills the CUs on 8x8 layers
    const bool w3 = wino3 && o.bf16x3 && !fused;                 // Winograd on the bf16 pipe, three exact pieces per operand; 16 / 17 / 20: persistent workgroups
    if (int rc = offer(w3, {CK_WINO3, CK_WINO3_K2, CK_WINO3P, CK_WINO3P_K2}, l.cot)) return rc;
    if (int rc = offer(w3 && few, {CK_WINO3_K4, CK_WINO3P_K4}, l.cot)) return rc;
    if (int rc = offer(w3 && fewer, {CK_WINO3_K8}, l.cot)) return rc;
    const bool w2 = wino3 && o.f16x2 && !l.raw && !fused;        // ... on the fp16 pipe, two-piece operands; the 4-way split where the three-piece kernel is offered it
    if (int rc = offer(w2, {CK_WINO2H, CK_WINO2H_K2}, l.cot)) return rc;
    if (int rc = offer(w2 && few, {CK_WINO2H_K4}, l.cot)) return rc;
    const bool w1 = wino3 && o.f16x1 && !l.raw && !fused;        // ... one-piece operands, the draft arithmetic: the same convs under the same guard (the 1x1
    if (int rc = offer(w1, {CK_WINO1H, CK_WINO1H_K2}, l.cot)) return rc;      // GEMMs and the attention have no one-piece form)
    if (int rc = offer(w1 && few, {CK_WINO1H_K4}, l.cot)) return rc;
    const bool g1 = l.ks == 1 && o.conv_dma1;                    // the 1x1 GEMMs, cout tiles of their own
    // small cout tiles first: the sweep of every 1x1 layer shape (profiles/r02_conv1x1_candidates.txt) has tiles 1-3 winning everywhere; 6 / 9 never did
    for (int id : {CK_DMA1, CK_DMA1_CK32}) {
        int tried = 0;
        for (int c : {2, 1, 3, 4, 6, 9})
            if (g1 && (l.CoutP / 32) % c == 0 && tried < 3 && usable(id, c)) {
                ++tried;
                if (int rc = emit(id, c)) return rc;
            }
    }
    for (int c = 4; c >= 1; --c)                                 // the split-operand GEMMs, cout tiles 4 .. 1: two fp16 pieces ...
        if (int rc = offer(g1 && o.f16x2 && !l.raw, {CK_GEMM1_F16X2}, c)) return rc;
    for (int c = 4; c >= 1; --c)                                 // ... three exact bf16 pieces
        if (int rc = offer(g1 && o.bf16x3, {CK_GEMM1_BF16X3}, c)) return rc;
    if (int rc = offer(g1, {CK_DMA1_PX64}, 1)) return rc;        // 256-pixel tiles, cout tiles 1 / 2
    return offer(g1 && (l.CoutP / 32) % 2 == 0, {CK_DMA1_PX64}, 2);
}

// the deepest K split the tuner can time for a layer: the K-split scratch is sized for it before the tuner runs (0: no split is offered)
constexpr int tuner_deepest_split(const TunerLayer& l, const TunerOptions& o) {
    int parts = 0;
    tuner_candidates(l, o, [](int, int) { return true; }, [&](int id, int) { parts = k_parts(id) > parts ? k_parts(id) : parts; return 0; });
    return parts;
}

// ---- the rule, checked: what a layer is offered where every kernel takes it ----
namespace conv_tuner_check {
struct List { int id[48], cot[48], n; };
constexpr List candidates(const TunerLayer& l, const TunerOptions& o) {
    List r{};
    tuner_candidates(l, o, [](int, int) { return true; }, [&](int id, int cot) { r.id[r.n] = id; r.cot[r.n] = cot; ++r.n; return 0; });
    return r;
}
constexpr bool offers(const List& c, std::initializer_list<int> ids) {       // any of `ids`
    for (int i = 0; i < c.n; ++i)
        for (int id : ids)
            if (c.id[i] == id) return true;
    return false;
}
constexpr bool offers_all(const List& c, std::initializer_list<int> ids) {
    for (int id : ids)
        if (!offers(c, {id})) return false;
    return true;
}
constexpr bool is(const List& c, std::initializer_list<int> ids, std::initializer_list<int> cots) {      // the whole list, in order
    if ((size_t)c.n != ids.size() || ids.size() != cots.size()) return false;
    for (int i = 0; i < c.n; ++i)
        if (c.id[i] != ids.begin()[i] || c.cot[i] != cots.begin()[i]) return false;
    return true;
}
constexpr bool offers_family_from(const List& c, ConvFamily f) {
    for (int i = 0; i < c.n; ++i)
        if (conv_kernel(c.id[i]).family >= f) return true;
    return false;
}
//                                 winograd dma1  bf16x3 f16x2  f16x1  spade_fuse wdma
constexpr TunerOptions kDefault = {true,    true, true,  false, false, false,     true};
constexpr TunerOptions kBothF16 = {true,    true, true,  true,  true,  false,     true};
constexpr TunerOptions kNoBf16 =  {true,    true, false, true,  true,  false,     true};
constexpr TunerOptions kFused =   {true,    true, true,  true,  true,  true,      true};
constexpr TunerOptions kNoWino =  {false,   true, true,  true,  true,  false,     true};
static_assert(kDefault.signature() == 39 && kBothF16.signature() == 111 && kFused.signature() == 127, "the signature's bits stay: tables are stamped with it");
//                                   ks H   W   B  Cin   Cout CoutP cot wino_cot raw    spade  alt
constexpr TunerLayer kNorm3 =       {3, 16, 16, 2, 256,  256, 256,  2,  2,       false, false, 0};      // a GroupNorm-ed 3x3
constexpr TunerLayer kRaw3 =        {3, 16, 16, 2, 256,  256, 256,  2,  2,       true,  false, 0};
constexpr TunerLayer kSpade3 =      {3, 16, 16, 2, 256,  256, 256,  2,  2,       false, true,  0};
constexpr TunerLayer kStem =        {3, 32, 32, 2, 10,   96,  96,   1,  1,       true,  false, CK_GEMM3_IM2COL};
constexpr TunerLayer kNorm1 =       {1, 16, 16, 2, 256,  384, 384,  2,  2,       false, false, 0};
constexpr TunerLayer kRaw1 =        {1, 16, 16, 2, 256,  384, 384,  2,  2,       true,  false, 0};
constexpr TunerLayer kWide3 =       {3, 8,  8,  64, 2304, 1152, 1152, 2, 2,      false, false, 0};      // above WINO_MAX_CIN; pairs = 32 * 18: 2 * pairs >= 1024
constexpr TunerLayer kBig3 =        {3, 32, 32, 64, 256, 256, 256,  2,  2,       false, false, 0};      // many pairs: no deep split

static_assert(is(candidates(kNorm3, kDefault), {0, 1, 2, 3, 4, 0, 1, 2, 3, 8, 10, 11, 16, 17, 18, 20, 19}, {2, 2, 2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2}),
              "a GroupNorm-ed 16 x 16 3x3 at B = 2, default options: the order");
static_assert(is(candidates(kNorm3, kBothF16), {0, 1, 2, 3, 4, 0, 1, 2, 3, 8, 10, 11, 16, 17, 18, 20, 19, 12, 13, 26, 24, 25, 27},
                 {2, 2, 2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}), "... under f16x2 and f16x1: the two-piece ids, then the one-piece ids");
static_assert(is(candidates(kBig3, kDefault), {0, 1, 2, 3, 4, 0, 1, 2, 3, 8, 10, 11, 16, 17}, {2, 2, 2, 2, 2, 1, 1, 1, 1, 2, 2, 2, 2, 2}),
              "many pairs: no 4- or 8-way split");
static_assert(offers_all(candidates(kRaw3, kBothF16), {4, 8, 10, 11, 16, 17}) && !offers(candidates(kRaw3, kBothF16), {12, 13, 26, 24, 25, 27}),
              "a raw-input 3x3 is offered no fp16 Winograd id");
static_assert(offers(candidates(kNorm1, kBothF16), {14}) && !offers(candidates(kRaw1, kBothF16), {14}) && offers(candidates(kRaw1, kBothF16), {15}),
              "a raw-input 1x1 is not offered the two-piece GEMM");
static_assert(!offers(candidates(kNorm3, kNoBf16), {10, 11, 16, 17, 18, 19, 20, 15}) && !offers(candidates(kNorm1, kNoBf16), {10, 11, 16, 17, 18, 19, 20, 15}) &&
              offers_all(candidates(kNorm3, kNoBf16), {4, 8, 12, 13, 26, 24, 25, 27}) && offers(candidates(kNorm1, kNoBf16), {14}),
              "bf16x3 off: nothing from 10 to 20 and no 15; the fp16 ids stay");
static_assert(is(candidates(kSpade3, kFused), {4, 8}, {2, 2}) && !offers_family_from(candidates(kSpade3, kFused), CF_WINO2H),
              "a fused SPADE loader: the fp32 Winograd kernel only, no split-operand id");
static_assert(offers_all(candidates(kSpade3, kBothF16), {0, 4, 10, 12, 24, 26, 27}), "an unfused SPADE norm: the materialised tensor is a normalised input");
static_assert(is(candidates(kStem, kDefault), {0, 1, 2, 3, 4, 23, 23, 23, 23, 8, 10, 11, 16, 17, 18, 20, 19}, {1, 1, 1, 1, 1, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1}),
              "the stem: one pass of tiles (cout tile 1), then its GEMM form at cout tiles 4 .. 1");
static_assert(is(candidates(kNorm1, kDefault), {0, 1, 2, 0, 1, 2, 5, 5, 5, 6, 6, 6, 15, 15, 15, 15, 9, 9}, {2, 2, 2, 1, 1, 1, 2, 1, 3, 2, 1, 3, 4, 3, 2, 1, 1, 2}) &&
              !offers_family_from(candidates(kNorm1, kBothF16), CF_WINO), "a 1x1: no Winograd id; the DMA GEMMs at cout tiles 2, 1, 3 and no further");
static_assert(offers_all(candidates(kWide3, kDefault), {18, 20}) && !offers(candidates(kWide3, kDefault), {19}) && 2 * tuner_pairs(kWide3) >= 1024 &&
              offers_all(candidates(kWide3, kBothF16), {26, 27}), "above WINO_MAX_CIN: the 4-way ids at every batch, the 8-way one on the terms of every other layer");
static_assert(!offers_family_from(candidates(kNorm3, kNoWino), CF_WINO) && tuner_deepest_split(kNorm3, kNoWino) == 0 &&
              tuner_deepest_split(kNorm3, {true, true, false, false, false, false, true}) == 2, "no 4- or 8-part id on offer: the scratch is sized for two parts");
static_assert(wino_needs_4_parts(2304) && !wino_needs_4_parts(2048), "layers the tuner offers four parts at every batch");

// the deepest split equals what ensure_ksplit computed by hand before the rule was stated here: 8 if 4 * pairs < 1024, else 4 if few pairs, else 2
// (bf16x3 and winograd on; B = 1 .. 128, a handful of CoutP; one assertion per plane and side of WINO_MAX_CIN keeps each evaluation short)
constexpr bool deepest_split_is_the_old_expression(int plane, int Cin) {
    for (int B = 1; B <= 128; ++B)
        for (int CoutP : {32, 96, 256, 1152, 2304}) {
            const TunerLayer l = {3, plane, plane, B, Cin, CoutP, CoutP, 2, CoutP % 64 == 0 ? 2 : 1, false, false, 0};
            const int want = 4 * tuner_pairs(l) < 1024 ? 8 : tuner_few_pairs(l) ? 4 : 2;
            if (tuner_deepest_split(l, kDefault) != want) return false;
        }
    return true;
}
static_assert(deepest_split_is_the_old_expression(8, 1024), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(8, WINO_MAX_CIN), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(8, WINO_MAX_CIN + 16), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(8, WINO_MAX_CIN_K4), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(16, 1024), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(16, WINO_MAX_CIN), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(16, WINO_MAX_CIN + 16), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
static_assert(deepest_split_is_the_old_expression(16, WINO_MAX_CIN_K4), "tuner_deepest_split disagrees with 8 / 4 / 2 by pairs");
}  // namespace conv_tuner_check

}  // namespace mcvd
