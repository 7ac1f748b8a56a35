// conv dispatch (tile-shape heuristic), the simple one-thread-per-output HIP kernel used to triangulate the
// MFMA kernel in tests, and the weight repacking kernel.
#include <stdlib.h>

#include "conv_mfma.h"
#include "../conv_kernels.h"

namespace mcvd {

int conv_cout_tile(int Cout) {
    if (Cout % 96 == 0) return 3;
    if (Cout % 128 == 0) return 4;
    if (Cout % 64 == 0) return 2;
    return 1;
}

int conv_chunk(int ks) { return ks == 3 ? 16 : 32; }   // packing granule of Cin (the largest chunk any tile shape uses)

#ifdef MCVD_DIAG
static int env_int(const char* name, int dflt) {      // diagnostics build only: the product library reads no environment on a launch path
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
#endif

// the kernel (conv_kernels.h: ConvKernel) the last launch_conv_mfma of this thread dispatched to: tests assert a forced id did not fall back silently
static thread_local int g_last_conv_kernel = -1;
int last_conv_kernel() { return g_last_conv_kernel; }

// partials per (sample, channel) the last conv launch of this thread wrote into a.stats (0: the kernel that ran does not emit)
static thread_local int g_last_stats_np = 0;
int last_conv_stats_np() { return g_last_stats_np; }
void set_last_conv_stats_np(int np) { g_last_stats_np = np; }

// 1: the last conv launch of this thread also wrote the (A, B) table of the norm over its output (ConvArgs::gno)
static thread_local int g_last_gn_fused = 0;
int last_conv_gn_fused() { return g_last_gn_fused; }
void set_last_conv_gn_fused(int v) { g_last_gn_fused = v; }

// the launch as the kernel sees it: its K parts in ksplit (the fp32 Winograd kernel without a split -- the last resort of every list -- takes
// the caller's arguments as they come)
static ConvArgs with_k_parts(const ConvKernelDesc& k, const ConvArgs& a) {
    ConvArgs b = a;
    if (k.id != CK_WINO) b.ksplit = k.kparts;
    return b;
}
static int dma1_chunk(int id) { return id == CK_DMA1_CK32 ? 32 : 16; }      // channels per chunk
static int dma1_pxw(int id) { return id == CK_DMA1_PX64 ? 2 : 1; }          // 2: 64 pixels per wave

// what the admission rule (conv_kernels.h: wino_admits) reads of a launch of `family` with a.ksplit = ksplit
static WinoLaunch wino_launch_of(ConvFamily family, const ConvArgs& a, int ksplit) {
    const float* w = family == CF_WINO ? a.wpw : (family == CF_WINO2H || family == CF_WINO1H) ? a.wph : a.wpb;
    return {a.ks, a.H, a.W, a.B, a.Cin, a.CinP, a.C0, a.C1, a.Cout, a.CoutP, wino_kernel_parts(family, ksplit), w != nullptr, a.gb != nullptr,
            a.part ? a.part_floats : 0};
}

int conv_wino_require(ConvFamily family, const ConvArgs& a, const char* what) {
    const int parts = wino_kernel_parts(family, a.ksplit);
    MCVD_REQUIRE(wino_admits(family, wino_launch_of(family, a, a.ksplit)),
                 "%s: unsupported (ks=%d H=%d W=%d Cin=%d C0=%d ksplit=%d, packed weights %s; Cin <= %d, %d channels per K part)", what, a.ks, a.H, a.W,
                 a.Cin, a.C0, a.ksplit, wino_launch_of(family, a, a.ksplit).weights ? "present" : "missing",
                 family == CF_WINO3P ? WINO_TABLE_CH : wino_max_cin(parts), family == CF_WINO3P ? WINO_TABLE_CH : wino_table_ch(a.H == 8 && a.W == 8));
    return 0;
}

// One usable / launch pair for every kernel the dispatcher serves, keyed by id.  The direct tiles (launch_conv_mfma's heuristic) and the GEMM
// forms of a 3x3 (model.cpp) are not launched from here: not usable.
bool conv_kernel_usable(int id, const ConvArgs& a) {
    const ConvKernelDesc& k = conv_kernel(id);
    switch (k.family) {
        case CF_WINO:
        case CF_WINO2H:
        case CF_WINO1H:
        case CF_WINO3:
        case CF_WINO3P: return wino_admits(k.family, wino_launch_of(k.family, a, k.id != CK_WINO ? k.kparts : a.ksplit));      // (with_k_parts)
        case CF_SPLIT1: return conv1x1_h2_supported(a, a.cot, k.pieces);
        case CF_DMA1: return conv1x1_dma_supported(a, dma1_chunk(id), dma1_pxw(id)) && !(id == CK_DMA1_CK32 && a.cot == 9);
        default: return false;
    }
}

int conv_kernel_launch(int id, const ConvArgs& a, hipStream_t s) {
    const ConvKernelDesc& k = conv_kernel(id);
    switch (k.family) {
        case CF_WINO: return launch_conv_wino(with_k_parts(k, a), s);
        case CF_WINO2H:
        case CF_WINO1H: return launch_conv_wino2h(with_k_parts(k, a), k.pieces, s);
        case CF_WINO3: return launch_conv_wino3(with_k_parts(k, a), s);
        case CF_WINO3P: return launch_conv_wino3p(with_k_parts(k, a), s);
        case CF_SPLIT1: return launch_conv1x1_h2(a, a.cot, s, k.pieces);
        case CF_DMA1: return launch_conv1x1_dma(a, a.cot, dma1_chunk(id), s, dma1_pxw(id));
        default: break;
    }
    MCVD_REQUIRE(false, "conv: kernel id %d is not launched by the dispatcher", id);
}

int launch_conv_mfma(const ConvArgs& a, hipStream_t s) {
    g_last_stats_np = 0;
    g_last_gn_fused = 0;
    MCVD_REQUIRE(a.ks == 1 || a.ks == 3, "conv: kernel size %d unsupported", a.ks);
    MCVD_REQUIRE(a.W >= 8 && (a.W & (a.W - 1)) == 0 && a.W <= 256, "conv: W=%d must be a power of two in [8,256]", a.W);
#ifdef MCVD_DIAG
    static const int forced = env_int("MCVD_CONV_SHAPE", -1);             // tile-heuristic experiments (tests/gpu_diag.py)
    static const int min_blocks = env_int("MCVD_CONV_MIN_BLOCKS", 400);
#else
    constexpr int forced = -1;              // (the "conv_shape" context option forces a kernel family; this is the direct kernel's tile)
    constexpr int min_blocks = 400;
#endif
    const long px = (long)a.B * a.H * a.W;
    const int ntc = a.CoutP / (32 * (a.cot > 0 ? a.cot : 1));
    auto blocks = [&](int bpx) { return ((px + bpx - 1) / bpx) * ntc; };
    auto fits = [&](int bpx) { return bpx % a.W == 0 && (bpx / a.W <= a.H ? a.H % (bpx / a.W) == 0 : (bpx / a.W) % a.H == 0); };
    int shape;
    // the hint's own kernel where it applies, else the next of its fallback list (conv_kernels.h), else the tile heuristic
    for (const int* f = conv_kernel(a.shape_hint).fallback; *f >= 0; ++f)
        if (conv_kernel_usable(*f, a)) { g_last_conv_kernel = *f; return conv_kernel_launch(*f, a, s); }
    if (a.cot < 1 || a.cot > 4 || a.CoutP % (32 * a.cot) != 0) {   // a cout tile meant for another kernel: use this one's
        ConvArgs b = a;
        b.cot = conv_cout_tile(a.Cout);
        if (a.CoutP % (32 * b.cot) != 0) b.cot = 1;
        return launch_conv_mfma(b, s);
    }
    const int want = conv_kernel(a.shape_hint).family == CF_TILE ? a.shape_hint : forced;
    if (want >= 0 && want <= 3 && fits(want == 0 ? 256 : want == 1 ? 128 : 64)) shape = want;
    else if (fits(256) && blocks(256) >= min_blocks) shape = 0;
    else if (fits(128) && blocks(128) >= min_blocks) shape = 1;
    else if (fits(64)) shape = 2;
    else if (fits(128)) shape = 1;
    else shape = 0;
    typedef int (*fn_t)(const ConvArgs&, int, hipStream_t);
    static const fn_t tab3[4] = {conv3_cot1, conv3_cot2, conv3_cot3, conv3_cot4};
    static const fn_t tab1[4] = {conv1_cot1, conv1_cot2, conv1_cot3, conv1_cot4};
    g_last_conv_kernel = shape;
    return (a.ks == 3 ? tab3 : tab1)[a.cot - 1](a, shape, s);
}

// ---------------------------------------------------------------------------------------------------------
// Naive direct convolution: one thread per output element, fp32 FMA chain in (ci, tap) order.
__global__ void conv_naive_kernel(ConvArgs a) {
    const long n = (long)a.B * a.Cout * a.H * a.W;
    const int HW = a.H * a.W;
    const int KK = a.ks * a.ks;
    const int pad = a.ks / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % a.W);
        const int y = (int)((i / a.W) % a.H);
        const int co = (int)((i / HW) % a.Cout);
        const int b = (int)(i / ((long)HW * a.Cout));
        float acc = 0.0f;
        for (int ci = 0; ci < a.Cin; ++ci) {
            const float* src = (ci < a.C0) ? a.x0 + ((long)b * a.C0 + ci) * HW : a.x1 + ((long)b * a.C1 + (ci - a.C0)) * HW;
            float ca = 1.0f, cb = 0.0f;
            if (a.coef) { ca = a.coef[((long)b * a.Cin + ci) * 2]; cb = a.coef[((long)b * a.Cin + ci) * 2 + 1]; }
            for (int t = 0; t < KK; ++t) {
                const int yy = y + t / a.ks - pad, xx = x + t % a.ks - pad;
                if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
                float v = src[yy * a.W + xx];
                if (a.coef) v = v * ca + cb;
                if (a.act) v = silu_f(v);
                acc = fmaf(a.wp[((long)ci * KK + t) * a.CoutP + co], v, acc);
            }
        }
        float v = acc + a.bias[co];
        if (a.res) v += a.res[i];
        a.y[i] = v * a.out_scale;
    }
}

int launch_conv_naive(const ConvArgs& a, hipStream_t s) {
    const long n = (long)a.B * a.Cout * a.H * a.W;
    const int blocks = (int)((n + 255) / 256 > 65535 * 8 ? 65535 * 8 : (n + 255) / 256);
    hipLaunchKernelGGL(conv_naive_kernel, dim3(blocks), dim3(256), 0, s, a);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// [Cout][Cin][ks][ks] (nn.Conv2d) or [Cin][Cout] (NIN.W, layers.py:538)  ->  wp[(ci*KK + tap)*CoutP + cout_off + co]
__global__ void pack_conv_weight_kernel(const float* w, float* wp, int Cout, int Cin, int KK, int CoutP, int nin,
                                        int cout_off) {
    const long n = (long)Cout * Cin * KK;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int co, ci, t;
        if (nin) {                    // i = ci*Cout + co
            co = (int)(i % Cout); ci = (int)(i / Cout); t = 0;
        } else {                      // i = (co*Cin + ci)*KK + t
            t = (int)(i % KK); ci = (int)((i / KK) % Cin); co = (int)(i / ((long)KK * Cin));
        }
        wp[((long)ci * KK + t) * CoutP + cout_off + co] = w[i];
    }
}

int launch_pack_conv_weight(const float* w, float* wp, int Cout, int Cin, int ks, int CinP, int CoutP, int nin,
                            int cout_off, hipStream_t s) {
    (void)CinP;
    const long n = (long)Cout * Cin * ks * ks;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(blocks), dim3(256), 0, s, w, wp, Cout, Cin, ks * ks, CoutP, nin,
                       cout_off);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mcvd
