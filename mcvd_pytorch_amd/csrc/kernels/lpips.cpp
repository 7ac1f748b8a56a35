// LPIPS of video_gen's test mode (runners/ncsn_runner.py:1427-1431, :1590-1591, :1602-1609; models/networks_basic.py:25-97,
// models/pretrained_networks.py:56-94, models/eval_models.py:35-37), version 0.1 on the AlexNet feature stack, on the device.
//
// Per frame, for the C channels of pred / real ([B, T*C, H, W] fp32 in [0, 1]):
//   u8   = x.mul(255).byte()                       ToPILImage (no MNIST rounding: LPIPS takes the un-rounded frame), .convert("RGB")
//   r    = Pillow resize((128, 128), BILINEAR)     horizontal pass, uint8 rows, vertical pass; 8-bit fixed-point taps with 22 fractional
//                                                  bits built on the host in double exactly as Pillow builds them (resize_table); a pass
//                                                  whose input length is 128 is skipped.  Integer arithmetic: bit-exact.
//   x    = ((r / 255 - 0.5) / 0.5 - shift) / scale ToTensor, Normalize, ScalingLayer: fp32, correctly rounded, in that order
//   taps = AlexNet features behind each ReLU       conv 3->64 k11 s4 p2 | pool 3/2, conv 64->192 k5 p2 | pool 3/2, conv 192->384 k3 p1 |
//                                                  conv 384->256 k3 p1 | conv 256->256 k3 p1
//   d_k  = mean_p sum_c lin_k[c] (f0/(|f0|+1e-10) - f1/(|f1|+1e-10))^2;   lpips = ((((d_1 + d_2) + d_3) + d_4) + d_5) in fp32
//
// Kernels: lpips_prep_h / lpips_prep_v (quantise + resize + normalise), conv_gemm_mfma_kernel (one general conv: implicit GEMM on
// v_mfma_f32_32x32x2_f32, any kernel size / stride / zero padding, pixels of all images flattened into the GEMM's N so that 7 x 7 maps
// fill tiles across the batch; bias + ReLU in the epilogue), maxpool3s2_kernel, lpips_distance_kernel (one workgroup per frame and tap,
// fp64 sums in a fixed order: bit-identical run to run).  Everything runs on the context's stream; nothing reads the environment.
#include "../lpips.h"
#include "../model.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace mcvd {

const LpipsLayer LPIPS_LAYERS[LPIPS_TAPS] = {
    {0, 1, 3, 64, 11, 4, 2, 128, 31, 0}, {3, 2, 64, 192, 5, 1, 2, 15, 15, 1}, {6, 3, 192, 384, 3, 1, 1, 7, 7, 1},
    {8, 4, 384, 256, 3, 1, 1, 7, 7, 0}, {10, 5, 256, 256, 3, 1, 1, 7, 7, 0}};

namespace {

typedef float cg_f32x16 __attribute__((ext_vector_type(16)));
typedef float cg_f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ general conv: implicit GEMM on the fp32 MFMA
// D[co][n] = sum_k Wp[k][co] * X[k][n]:  A operand = weights (rows = output channels), B operand = the im2col of the input, gathered on the
// fly (k = (ci * ks + ky) * ks + kx; n = image * OH * OW + oy * OW + ox), so an accumulator register holds 32 consecutive output pixels
// of one channel across lanes and the NCHW stores are contiguous runs.  Workgroup = 4 wave64 = 64 output channels x 128 pixels, each
// wave 64 x 32 (two accumulators); K in chunks of 16, double-buffered in LDS with a register prefetch of chunk i + 1 under the MFMAs of
// chunk i: one barrier per chunk.  Per output the k order is fixed (0 .. K-1, one fma chain): results do not depend on the tiling.
constexpr int CG_BM = 64, CG_BN = 128, CG_KC = 16, CG_THREADS = 256;

struct ConvGemmArgs {
    const float* x;
    const float* wp;
    const float* bias;      // [Cout] or null
    float* y;
    int Cin, H, W, Cout, CoutP, ks, stride, pad, OH, OW, K, KP, relu;
    long long Ntot;         // images * OH * OW
};

__global__ __launch_bounds__(CG_THREADS) void conv_gemm_mfma_kernel(ConvGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float sW[2][CG_KC][CG_BM];
    __shared__ float sX[2][CG_KC][CG_BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long n0 = (long long)blockIdx.x * CG_BN;
    const int co0 = blockIdx.y * CG_BM;
    const int OHW = a.OH * a.OW, HW = a.H * a.W, ks = a.ks;

    // gather role: this thread stages pixel gp of the tile for the k rows gk, gk + 2, ..., gk + 14 of every chunk
    const int gp = tid & (CG_BN - 1), gk = tid >> 7;
    const long long gn = n0 + gp;
    const bool gvalid = gn < a.Ntot;
    const long long gb = gvalid ? gn / OHW : 0;
    const int gpix = gvalid ? (int)(gn - gb * OHW) : 0;
    const int goy = gpix / a.OW, gox = gpix - goy * a.OW;
    const int iy0 = goy * a.stride - a.pad, ix0 = gox * a.stride - a.pad;
    const float* xb = a.x + gb * (long long)a.Cin * HW;
    int knext = gk, kci = 0, kky = 0, kkx = gk;      // (ci, ky, kx) of k = knext, advanced by 2 per staged element across all chunks
#define CG_NORM_K()                            \
    while (kkx >= ks) { kkx -= ks; ++kky; }    \
    while (kky >= ks) { kky -= ks; ++kci; }
    CG_NORM_K()
    const int wr = tid >> 4, wc = (tid & 15) * 4;      // weight role: row wr of the chunk, columns wc .. wc + 3

    float rx[CG_KC / 2];
    cg_f32x4 rw;
    // loads are unconditional (a dead element reads the image's first value and is discarded): no branch around a load
#define CG_LOAD(ch)                                                                                                 \
    {                                                                                                               \
        _Pragma("unroll") for (int j = 0; j < CG_KC / 2; ++j) {                                                     \
            const int iy = iy0 + kky, ix = ix0 + kkx;                                                               \
            const bool ok = gvalid && knext < a.K && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;                    \
            const int off = ok ? (kci * a.H + iy) * a.W + ix : 0;                                                   \
            const float v = xb[off];                                                                                \
            rx[j] = ok ? v : 0.0f;                                                                                  \
            knext += 2;                                                                                             \
            kkx += 2;                                                                                               \
            CG_NORM_K()                                                                                             \
        }                                                                                                           \
        rw = *reinterpret_cast<const cg_f32x4*>(a.wp + (long long)((ch) * CG_KC + wr) * a.CoutP + co0 + wc);        \
    }
#define CG_STORE(buf)                                                                          \
    {                                                                                          \
        _Pragma("unroll") for (int j = 0; j < CG_KC / 2; ++j) sX[buf][gk + 2 * j][gp] = rx[j]; \
        *reinterpret_cast<cg_f32x4*>(&sW[buf][wr][wc]) = rw;                                   \
    }

    cg_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }

    const int nch = a.KP / CG_KC;
    CG_LOAD(0)
    CG_STORE(0)
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) CG_LOAD(ch + 1)
#pragma unroll
        for (int kp = 0; kp < CG_KC / 2; ++kp) {
            const float a0 = sW[buf][2 * kp + half][l31], a1 = sW[buf][2 * kp + half][32 + l31];
            const float bx = sX[buf][2 * kp + half][wave * 32 + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bx, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bx, acc1, 0, 0, 0);
        }
        if (ch + 1 < nch) CG_STORE(buf ^ 1)      // the other buffer: every wave passed the barrier behind its last reads of it
        __syncthreads();
    }
#undef CG_LOAD
#undef CG_STORE
#undef CG_NORM_K

    // epilogue: bias, ReLU, NCHW stores (lanes 0-31 of a register: 32 consecutive pixels of one channel)
    const long long en = n0 + wave * 32 + l31;
    if (en >= a.Ntot) return;
    const long long eb = en / OHW;
    const int epix = (int)(en - eb * OHW);
    float* yb = a.y + eb * (long long)a.Cout * OHW + epix;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co < a.Cout) {
                float v = (ct ? acc1[r] : acc0[r]) + (a.bias ? a.bias[co] : 0.0f);
                if (a.relu) v = fmaxf(v, 0.0f);
                yb[(long long)co * OHW] = v;
            }
        }
}

__global__ __launch_bounds__(256) void pack_conv_gemm_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int K, int CoutP) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)Cout * K) return;
    const int co = (int)(i / K), k = (int)(i - (long long)co * K);
    wp[(long long)k * CoutP + co] = w[i];
}

__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W, int OH,
                                                          int OW) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const long long nc = i / ((long long)OW * OH);
    const float* p = x + nc * H * W + (long long)(2 * oy) * W + 2 * ox;      // rows 2 oy .. 2 oy + 2 <= H - 1 by the choice of OH
    float m = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, p[dy * W + dx]);
    y[i] = m;
}

// ------------------------------------------------------------------ quantise, resize, normalise
constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow: 8-bit pixels, 2 bits of headroom, 22 fractional bits

// x.mul(255).byte().  Inputs are in [0, 1]; the clamp only defines what lies outside.
__device__ __forceinline__ int quant255(float x) {
    const float v = __fmul_rn(x, 255.0f);
    return (int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// rows[img][c][y][ox]: the quantised frame after the horizontal pass (tab == null: W is 128, quantise only); img < nf: pred, else real.
// tab = first tap [128] | tap count [128] | coefficients [128][ksize]
__global__ __launch_bounds__(256) void lpips_prep_h_kernel(const float* __restrict__ pred, const float* __restrict__ real, int nf, int C, int H, int W,
                                                            const int* __restrict__ tab, int ksize, unsigned char* __restrict__ rows,
                                                            long long total) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % LPIPS_SIZE), y = (int)((i / LPIPS_SIZE) % H), c = (int)((i / ((long long)LPIPS_SIZE * H)) % C);
    const long long img = i / ((long long)LPIPS_SIZE * H * C);
    const float* src = (img < nf ? pred + img * C * H * W : real + (img - nf) * C * H * W) + ((long long)c * H + y) * W;
    int u;
    if (tab) {
        const int first = tab[ox], n = tab[LPIPS_SIZE + ox];
        const int* k = tab + 2 * LPIPS_SIZE + ox * ksize;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) ss += quant255(src[first + t]) * k[t];
        u = min(max(ss >> PRECISION_BITS, 0), 255);
    } else {
        u = quant255(src[ox]);
    }
    rows[i] = (unsigned char)u;
}

struct Scaling { float shift[3], scale[3]; };

// img[im][c3][oy][ox] fp32: the vertical pass (tab == null: H is 128), RGB replication of a one-channel frame, ToTensor, Normalize and
// the ScalingLayer; resized (test aid, may be null): [2][frames of the whole call][C][128][128] uint8, this chunk's first frame at `resized`
__global__ __launch_bounds__(256) void lpips_prep_v_kernel(const unsigned char* __restrict__ rows, int nf, int C, int H, const int* __restrict__ tab,
                                                            int ksize, Scaling sc, float* __restrict__ img, unsigned char* __restrict__ resized,
                                                            long long which_stride, long long total) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    constexpr int S = LPIPS_SIZE;
    const int ox = (int)(i % S), oy = (int)((i / S) % S), c3 = (int)((i / (S * S)) % 3);
    const long long im = i / (3LL * S * S);
    const int cc = C == 1 ? 0 : c3;
    const unsigned char* col = rows + ((im * C + cc) * H) * S + ox;
    int u;
    if (tab) {
        const int first = tab[oy], n = tab[S + oy];
        const int* k = tab + 2 * S + oy * ksize;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) ss += (int)col[(long long)(first + t) * S] * k[t];
        u = min(max(ss >> PRECISION_BITS, 0), 255);
    } else {
        u = (int)col[(long long)oy * S];
    }
    if (resized && c3 < C) {
        const long long which = im >= nf ? 1 : 0, f = im - which * nf;
        resized[which * which_stride + (f * C + c3) * S * S + oy * S + ox] = (unsigned char)u;
    }
    float x = __fdiv_rn((float)u, 255.0f);                             // ToTensor
    x = __fdiv_rn(__fsub_rn(x, 0.5f), 0.5f);                           // Normalize(0.5, 0.5)
    img[i] = __fdiv_rn(__fsub_rn(x, sc.shift[c3]), sc.scale[c3]);      // ScalingLayer
}

// ------------------------------------------------------------------ distance of one tap
// One workgroup per frame.  feat: [2 nf][C][HW] (image f: pred, image nf + f: real).  256 threads = PXB pixels x 256 / PXB channel
// slices; per pixel the two squared norms, then sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, all in fp64 and added in a
// fixed order (slices in index order, pixels per thread in index order, then a tree over threads).  per_tap[f][tap] = (float)(sum / HW);
// the last tap's launch also adds the five values in tap order in fp32 (val = res[0]; val += res[l], networks_basic.py:81-83).
__global__ __launch_bounds__(256) void lpips_distance_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int nf, int C, int HW,
                                                              int PXB, int tap, float* __restrict__ per_tap, float* __restrict__ out) {
    __shared__ double r0[256], r1[256];
    const int tid = threadIdx.x, px = tid % PXB, cs = tid / PXB, CS = 256 / PXB;
    const long long f = blockIdx.x;
    const float* f0 = feat + f * C * HW;
    const float* f1 = feat + (f + nf) * C * HW;
    double acc = 0.0;
    for (int p0 = 0; p0 < HW; p0 += PXB) {
        const int p = p0 + px;
        const bool ok = p < HW;
        double s0 = 0.0, s1 = 0.0;
        if (ok)
            for (int c = cs; c < C; c += CS) {
                const double u = (double)f0[(long long)c * HW + p], v = (double)f1[(long long)c * HW + p];
                s0 += u * u;
                s1 += v * v;
            }
        r0[tid] = s0;
        r1[tid] = s1;
        __syncthreads();
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < CS; ++k) { t0 += r0[k * PXB + px]; t1 += r1[k * PXB + px]; }
        __syncthreads();
        const double i0 = 1.0 / (sqrt(t0) + 1e-10), i1 = 1.0 / (sqrt(t1) + 1e-10);
        double d = 0.0;
        if (ok)
            for (int c = cs; c < C; c += CS) {
                const double u = (double)f0[(long long)c * HW + p] * i0 - (double)f1[(long long)c * HW + p] * i1;
                d += (double)lin[c] * (u * u);
            }
        r0[tid] = d;
        __syncthreads();
        if (cs == 0 && ok)
            for (int k = 0; k < CS; ++k) acc += r0[k * PXB + px];
        __syncthreads();
    }
    r0[tid] = cs == 0 ? acc : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) r0[tid] += r0[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float v = (float)(r0[0] / (double)HW);
        per_tap[f * LPIPS_TAPS + tap] = v;
        if (tap == LPIPS_TAPS - 1) {
            float val = per_tap[f * LPIPS_TAPS];
            for (int l = 1; l < LPIPS_TAPS - 1; ++l) val = __fadd_rn(val, per_tap[f * LPIPS_TAPS + l]);
            out[f] = __fadd_rn(val, v);
        }
    }
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter (support 1), one axis, in_size -> 128: the same expressions
// in the same order in double (this file is compiled without fp contraction).  Layout as the prep kernels read it.
std::vector<int> resize_table(int in_size, int* ksize_out) {
    const int out_size = LPIPS_SIZE;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<int> tab((size_t)2 * out_size + (size_t)out_size * ksize, 0);
    std::vector<double> w((size_t)ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double v = (x + xmin - center + 0.5) * ss;
            if (v < 0.0) v = -v;
            w[x] = v < 1.0 ? 1.0 - v : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            tab[(size_t)2 * out_size + (size_t)xx * ksize + x] =
                w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PRECISION_BITS)) : (int)(0.5 + w[x] * (1 << PRECISION_BITS));
        }
        tab[xx] = xmin;
        tab[out_size + xx] = xmax;
    }
    *ksize_out = ksize;
    return tab;
}

// where each buffer of the chunk workspace starts (in floats, for a workspace of `cap` frames)
struct WsLayout {
    long long img, tap[LPIPS_TAPS], pool[2], per_tap, total;
    explicit WsLayout(long long cap) {
        long long o = 0;
        img = o; o += cap * 2 * 3 * LPIPS_SIZE * LPIPS_SIZE;
        int np = 0;
        for (int k = 0; k < LPIPS_TAPS; ++k) {
            const LpipsLayer& L = LPIPS_LAYERS[k];
            if (L.pool) { pool[np++] = o; o += cap * 2 * L.Cin * L.H * L.H; }
            tap[k] = o; o += cap * 2 * L.Cout * L.OH * L.OH;
        }
        per_tap = o; o += cap * LPIPS_TAPS;
        total = o;
    }
};

}  // namespace

int conv_gemm_kp(int Cin, int ks) { return round_up(Cin * ks * ks, CG_KC); }
int conv_gemm_coutp(int Cout) { return round_up(Cout, CG_BM); }

int launch_pack_conv_gemm(const float* w, float* wp, int Cout, int Cin, int ks, hipStream_t s) {
    const int K = Cin * ks * ks, KP = conv_gemm_kp(Cin, ks), CoutP = conv_gemm_coutp(Cout);
    MCVD_HIP_CHECK(hipMemsetAsync(wp, 0, (size_t)KP * CoutP * sizeof(float), s));
    const long long n = (long long)Cout * K;
    hipLaunchKernelGGL(pack_conv_gemm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, wp, Cout, K, CoutP);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_conv_gemm(const float* x, const float* wp, const float* bias, float* y, int N, int Cin, int H, int W, int Cout, int ks, int stride,
                     int pad, int relu, hipStream_t s) {
    MCVD_REQUIRE(x && wp && y, "conv2d_strided: NULL argument");
    MCVD_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "conv2d_strided: bad shape");
    MCVD_REQUIRE(ks >= 1 && (ks & 1) && stride >= 1 && pad >= 0, "conv2d_strided: ks = %d (odd), stride = %d, pad = %d", ks, stride, pad);
    MCVD_REQUIRE(H + 2 * pad >= ks && W + 2 * pad >= ks, "conv2d_strided: the %d x %d kernel exceeds the padded %d x %d input", ks, ks, H, W);
    ConvGemmArgs a;
    a.x = x; a.wp = wp; a.bias = bias; a.y = y;
    a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.CoutP = conv_gemm_coutp(Cout); a.ks = ks; a.stride = stride; a.pad = pad;
    a.OH = (H + 2 * pad - ks) / stride + 1;
    a.OW = (W + 2 * pad - ks) / stride + 1;
    a.K = Cin * ks * ks; a.KP = conv_gemm_kp(Cin, ks); a.relu = relu;
    a.Ntot = (long long)N * a.OH * a.OW;
    MCVD_REQUIRE((long long)Cin * H * W < (1LL << 31) && (long long)Cin * ks * ks < (1LL << 30), "conv2d_strided: an image exceeds 32-bit offsets");
    const long long tiles = (a.Ntot + CG_BN - 1) / CG_BN;
    MCVD_REQUIRE(tiles < (1LL << 31) && a.CoutP / CG_BM < 65536, "conv2d_strided: %lld pixel tiles exceed one launch", tiles);
    hipLaunchKernelGGL(conv_gemm_mfma_kernel, dim3((unsigned)tiles, (unsigned)(a.CoutP / CG_BM)), dim3(CG_THREADS), 0, s, a);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_maxpool3s2(const float* x, float* y, long long NC, int H, int W, hipStream_t s) {
    MCVD_REQUIRE(H >= 3 && W >= 3, "maxpool: %d x %d map", H, W);
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const long long total = NC * OH * OW;
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, total, H, W, OH, OW);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ the net
static void param_names(int k, char* slice_w, char* slice_b, char* feat_w, char* feat_b, char* lin, size_t n) {
    const LpipsLayer& L = LPIPS_LAYERS[k];
    snprintf(slice_w, n, "net.slice%d.%d.weight", L.slice, L.feat);
    snprintf(slice_b, n, "net.slice%d.%d.bias", L.slice, L.feat);
    snprintf(feat_w, n, "features.%d.weight", L.feat);
    snprintf(feat_b, n, "features.%d.bias", L.feat);
    snprintf(lin, n, "lin%d.model.1.weight", k);
}

int lpips_set_param(mcvd_lpips* n, const char* name, const float* host, int64_t numel) {
    std::vector<float>* dst = nullptr;
    int64_t want = 0;
    for (int k = 0; k < LPIPS_TAPS && !dst; ++k) {
        const LpipsLayer& L = LPIPS_LAYERS[k];
        char sw[64], sb[64], fw[64], fb[64], ln[64];
        param_names(k, sw, sb, fw, fb, ln, sizeof(sw));
        if (!strcmp(name, sw) || !strcmp(name, fw)) { dst = &n->w[k]; want = (int64_t)L.Cout * L.Cin * L.ks * L.ks; }
        else if (!strcmp(name, sb) || !strcmp(name, fb)) { dst = &n->b[k]; want = L.Cout; }
        else if (!strcmp(name, ln)) { dst = &n->lin[k]; want = L.Cout; }
    }
    if (!dst && !strcmp(name, "scaling_layer.shift")) { dst = &n->shift; want = 3; }
    if (!dst && !strcmp(name, "scaling_layer.scale")) { dst = &n->scale; want = 3; }
    MCVD_REQUIRE(dst, "lpips_set_param: unknown parameter '%s'", name);
    MCVD_REQUIRE(numel == want, "lpips_set_param: '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)want);
    dst->assign(host, host + numel);
    n->finalized = false;
    return 0;
}

int lpips_finalize(mcvd_lpips* n) {
    hipStream_t s = n->ctx->stream;
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        char sw[64], sb[64], fw[64], fb[64], ln[64];
        param_names(k, sw, sb, fw, fb, ln, sizeof(sw));
        if (n->w[k].empty()) { set_error("lpips_finalize: missing %s (torchvision: %s)", sw, fw); return MCVD_ESTATE; }
        if (n->b[k].empty()) { set_error("lpips_finalize: missing %s (torchvision: %s)", sb, fb); return MCVD_ESTATE; }
    }
    for (int k = 0; k < LPIPS_TAPS; ++k)
        if (n->lin[k].empty()) { set_error("lpips_finalize: missing lin%d.model.1.weight", k); return MCVD_ESTATE; }
    if (n->shift.empty()) { set_error("lpips_finalize: missing scaling_layer.shift"); return MCVD_ESTATE; }
    if (n->scale.empty()) { set_error("lpips_finalize: missing scaling_layer.scale"); return MCVD_ESTATE; }

    size_t total = 0, raw_max = 0;
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        const LpipsLayer& L = LPIPS_LAYERS[k];
        total += (size_t)conv_gemm_kp(L.Cin, L.ks) * conv_gemm_coutp(L.Cout) + 2 * (size_t)round_up(L.Cout, 4);
        raw_max = std::max(raw_max, n->w[k].size());
    }
    MCVD_HIP_CHECK(hipStreamSynchronize(s));
    if (n->params) MCVD_HIP_CHECK(hipFree(n->params));
    n->params = nullptr;
    MCVD_HIP_CHECK(hipMalloc((void**)&n->params, total * sizeof(float)));
    float* raw = nullptr;
    MCVD_HIP_CHECK(hipMalloc((void**)&raw, raw_max * sizeof(float)));
    float* o = n->params;
    int rc = 0;
    for (int k = 0; k < LPIPS_TAPS && !rc; ++k) {
        const LpipsLayer& L = LPIPS_LAYERS[k];
        n->wp[k] = o; o += (size_t)conv_gemm_kp(L.Cin, L.ks) * conv_gemm_coutp(L.Cout);
        n->bias[k] = o; o += round_up(L.Cout, 4);
        n->lind[k] = o; o += round_up(L.Cout, 4);
        hipError_t e = hipMemcpyAsync(raw, n->w[k].data(), n->w[k].size() * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n->bias[k], n->b[k].data(), (size_t)L.Cout * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n->lind[k], n->lin[k].data(), (size_t)L.Cout * sizeof(float), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { set_error("lpips_finalize: upload failed: %s", hipGetErrorString(e)); rc = MCVD_EHIP; break; }
        rc = launch_pack_conv_gemm(raw, n->wp[k], L.Cout, L.Cin, L.ks, s);
        if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("lpips_finalize: synchronize failed"); rc = MCVD_EHIP; }      // `raw` is reused
    }
    (void)hipFree(raw);
    if (rc) return rc;
    for (int c = 0; c < 3; ++c) { n->sh[c] = n->shift[c]; n->sc[c] = n->scale[c]; }
    n->finalized = true;
    return 0;
}

static int resize_tab(mcvd_lpips* n, int in_size, const int** tab, int* ksize) {
    *tab = nullptr;
    *ksize = 0;
    if (in_size == LPIPS_SIZE) return 0;      // Pillow skips a pass whose input and output length agree
    auto it = n->tabs.find(in_size);
    if (it == n->tabs.end()) {
        int ks = 0;
        const std::vector<int> host = resize_table(in_size, &ks);
        int* dev = nullptr;
        MCVD_HIP_CHECK(hipMalloc((void**)&dev, host.size() * sizeof(int)));
        MCVD_HIP_CHECK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, n->ctx->stream));
        MCVD_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));      // `host` goes out of scope
        it = n->tabs.emplace(in_size, std::make_pair(dev, ks)).first;
    }
    *tab = it->second.first;
    *ksize = it->second.second;
    return 0;
}

int lpips_frames(mcvd_lpips* n, const float* pred01, const float* real01, int B, int T, int C, int H, int W, float* lpips_out,
                 unsigned char* resized_out, float* per_tap_out) {
    hipStream_t s = n->ctx->stream;
    const long long nfr = (long long)B * T;
    const int cap = (int)std::min<long long>(nfr, LPIPS_CHUNK);
    if (n->ws_frames < cap) {
        MCVD_HIP_CHECK(hipStreamSynchronize(s));
        if (n->ws) MCVD_HIP_CHECK(hipFree(n->ws));
        n->ws = nullptr;
        n->ws_frames = 0;
        MCVD_HIP_CHECK(hipMalloc((void**)&n->ws, (size_t)WsLayout(cap).total * sizeof(float)));
        n->ws_frames = cap;
    }
    const size_t rows_need = (size_t)cap * 2 * C * H * LPIPS_SIZE;
    if (n->rows_bytes < rows_need) {
        MCVD_HIP_CHECK(hipStreamSynchronize(s));
        if (n->rows) MCVD_HIP_CHECK(hipFree(n->rows));
        n->rows = nullptr;
        n->rows_bytes = 0;
        MCVD_HIP_CHECK(hipMalloc((void**)&n->rows, rows_need));
        n->rows_bytes = rows_need;
    }
    const int *tab_w, *tab_h;
    int ks_w, ks_h;
    if (int rc = resize_tab(n, W, &tab_w, &ks_w)) return rc;
    if (int rc = resize_tab(n, H, &tab_h, &ks_h)) return rc;
    const WsLayout lay(n->ws_frames);
    Scaling sc;
    for (int c = 0; c < 3; ++c) { sc.shift[c] = n->sh[c]; sc.scale[c] = n->sc[c]; }
    const long long frame_in = (long long)C * H * W, plane = (long long)LPIPS_SIZE * LPIPS_SIZE;

    for (long long f0 = 0; f0 < nfr; f0 += cap) {
        const int nf = (int)std::min<long long>(cap, nfr - f0);
        const long long nimg = 2LL * nf;
        float* img = n->ws + lay.img;
        {
            const long long total = nimg * C * H * LPIPS_SIZE;
            hipLaunchKernelGGL(lpips_prep_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pred01 + f0 * frame_in,
                               real01 + f0 * frame_in, nf, C, H, W, tab_w, ks_w, n->rows, total);
            MCVD_HIP_CHECK(hipGetLastError());
            const long long total_v = nimg * 3 * plane;
            hipLaunchKernelGGL(lpips_prep_v_kernel, dim3((unsigned)((total_v + 255) / 256)), dim3(256), 0, s, n->rows, nf, C, H, tab_h, ks_h, sc, img,
                               resized_out ? resized_out + f0 * C * plane : nullptr, nfr * C * plane, total_v);
            MCVD_HIP_CHECK(hipGetLastError());
        }
        float* per_tap = per_tap_out ? per_tap_out + f0 * LPIPS_TAPS : n->ws + lay.per_tap;
        const float* x = img;
        int np = 0;
        for (int k = 0; k < LPIPS_TAPS; ++k) {
            const LpipsLayer& L = LPIPS_LAYERS[k];
            if (L.pool) {
                const LpipsLayer& P = LPIPS_LAYERS[k - 1];
                float* pooled = n->ws + lay.pool[np++];
                if (int rc = launch_maxpool3s2(x, pooled, nimg * P.Cout, P.OH, P.OH, s)) return rc;
                x = pooled;
            }
            float* y = n->ws + lay.tap[k];
            if (int rc = launch_conv_gemm(x, n->wp[k], n->bias[k], y, (int)nimg, L.Cin, L.H, L.H, L.Cout, L.ks, L.stride, L.pad, 1, s)) return rc;
            const int HW = L.OH * L.OH;
            const int PXB = HW > 128 ? 256 : (HW > 64 ? 128 : 64);
            hipLaunchKernelGGL(lpips_distance_kernel, dim3((unsigned)nf), dim3(256), 0, s, y, n->lind[k], nf, L.Cout, HW, PXB, k, per_tap,
                               lpips_out + f0);
            MCVD_HIP_CHECK(hipGetLastError());
            x = y;
        }
    }
    return 0;
}

}  // namespace mcvd

mcvd_lpips::~mcvd_lpips() {
    if (params) (void)hipFree(params);
    if (ws) (void)hipFree(ws);
    if (rows) (void)hipFree(rows);
    for (auto& kv : tabs) (void)hipFree(kv.second.first);
}
