// The FID InceptionV3 (evaluation/inception.py: InceptionV3 :16-163, fid_inception_v3 :184-208, the patched blocks :211-328) on the device:
// the detector of fast_fid, fid_pr and nearest_neighbors.  The weights come from the caller (mcvd_inception_set_param, by the key names of
// pt_inception-2015-12-05-6726825d.pth); the package holds none.
//
//   x    = F.interpolate(images, (299, 299), bilinear, align_corners=False); 2 x - 1     inception_prep_kernel: per-axis tables from the host
//                                                                                        (fvd.cpp's coordinate rule and lerp order), any H, W
//   94 x   BasicConv2d = conv (no bias) + BatchNorm(eps 0.001, eval) + ReLU              conv_rect_mfma_kernel: relu(fma(acc, alpha, beta)),
//                                                                                        alpha = w / sqrt(var + 0.001), beta = b - mean alpha
//                                                                                        formed in fp64 on the host and rounded once
//   torch.cat of a block's branches                                                      no pass: every branch stores its channel slice
//   F.avg_pool2d(3, 1, 1, count_include_pad=False), F.max_pool2d(3, 1, 1)                pool3_kernel
//   MaxPool2d(3, 2)                                                                      launch_maxpool3s2 (lpips.cpp)
//   AdaptiveAvgPool2d((1, 1))                                                            global_avg_kernel: fp64 sum in index order
//
// conv_rect_mfma_kernel is conv_gemm_mfma_kernel's scheme (lpips.cpp) for rectangular kernels: D[co][n] = sum_k Wp[k][co] X[k][n] on
// v_mfma_f32_32x32x2_f32 -- exact fp32 products, per output ONE fma chain in the fixed order k = 0 .. K-1, so a result does not depend on
// the tile, on the other images of the batch or on the chunking.  Workgroup = 4 wave64 = BM output channels x 128 pixels (BM = 64, or 32
// for layers of at most 32 output channels: the two stem layers at 149 x 149 and 147 x 147 would otherwise run half their MFMAs on
// padding), K in chunks of 32, double-buffered in LDS (2 x 32 x (BM + 128) floats: 48 KB) with a register prefetch of chunk i + 1 under the
// MFMAs of chunk i.  On the 17 x 17 and 8 x 8 maps a chunk of images gives fewer workgroups than the device has compute units, so a
// workgroup runs alone and a K chunk costs one load latency whatever its depth: 32 rows halve the number of such waits against 16.  k -> (ci, ky, kx) comes from a per-layer table built on the host (one scalar load per k row, no div / mod in the
// gather); a 1 x 1 layer (stride 1, no padding) takes the path whose B operand is the plain strided load x[k][pixel].
// Everything runs on the context's stream; nothing reads the environment.
#include "../inception.h"
#include "../lpips.h"
#include "../model.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace mcvd {
namespace {

typedef float rc_f32x16 __attribute__((ext_vector_type(16)));
typedef float rc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RC_BN = 128, RC_KC = 32, RC_THREADS = 256;

struct ConvRectArgs {
    const float* x;
    const float* wp;
    const int* tab;         // [KP]: ci << 8 | ky << 4 | kx, -1 beyond K
    const float* alpha;     // [Cout] or null (1)
    const float* beta;      // [Cout] or null (0)
    float* y;
    int Cin, H, W, Cout, CoutP, stride, ph, pw, OH, OW, K, KP, relu, c0, Ctot;
    long long Ntot;         // images * OH * OW
};

template <int BM, bool ONE>
__global__ __launch_bounds__(RC_THREADS) void conv_rect_mfma_kernel(ConvRectArgs a) {
    __shared__ __attribute__((aligned(16))) float sW[2][RC_KC][BM];
    __shared__ float sX[2][RC_KC][RC_BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long n0 = (long long)blockIdx.x * RC_BN;
    const int co0 = blockIdx.y * BM;
    const int OHW = a.OH * a.OW, HW = a.H * a.W;

    // gather role: this thread stages pixel gp of the tile for the k rows gk, gk + 2, ..., gk + 30 of every chunk (gk is wave-uniform)
    const int gp = tid & (RC_BN - 1), gk = __builtin_amdgcn_readfirstlane(tid >> 7);
    const long long gn = n0 + gp;
    const bool gvalid = gn < a.Ntot;
    const long long gb = gvalid ? gn / OHW : 0;
    const int gpix = gvalid ? (int)(gn - gb * OHW) : 0;
    const int goy = gpix / a.OW, gox = gpix - goy * a.OW;
    const int iy0 = goy * a.stride - a.ph, ix0 = gox * a.stride - a.pw;
    const float* xb = a.x + gb * (long long)a.Cin * HW;
    // weight role: rows wr, wr + WROWS, ... of the chunk, columns wc .. wc + 3 (BM = 64: 16 rows per pass, two passes; BM = 32: one pass)
    constexpr int WQ = BM / 4, WROWS = RC_THREADS / WQ, WPASS = RC_KC / WROWS;
    static_assert(WPASS >= 1 && WPASS * WROWS == RC_KC, "the weight role must cover the chunk");
    const int wr = tid / WQ, wc = (tid % WQ) * 4;

    float rx[RC_KC / 2];
    rc_f32x4 rw[WPASS];
    // loads are unconditional (a dead element reads the image's first value and is discarded): no branch around a load
#define RC_LOAD(ch)                                                                                                  \
    {                                                                                                                \
        _Pragma("unroll") for (int j = 0; j < RC_KC / 2; ++j) {                                                      \
            const int k = (ch) * RC_KC + gk + 2 * j;                                                                 \
            bool ok;                                                                                                 \
            int off;                                                                                                 \
            if (ONE) {                                                                                               \
                ok = gvalid && k < a.K;                                                                              \
                off = k * HW + gpix;                                                                                 \
            } else {                                                                                                 \
                const int t = a.tab[k];                                                                              \
                const int iy = iy0 + ((t >> 4) & 15), ix = ix0 + (t & 15);                                           \
                ok = gvalid && t >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;                                 \
                off = (t >> 8) * HW + iy * a.W + ix;                                                                 \
            }                                                                                                        \
            const float v = xb[ok ? off : 0];                                                                        \
            rx[j] = ok ? v : 0.0f;                                                                                   \
        }                                                                                                            \
        _Pragma("unroll") for (int q = 0; q < WPASS; ++q)                                                            \
            rw[q] = *reinterpret_cast<const rc_f32x4*>(a.wp + (long long)((ch) * RC_KC + q * WROWS + wr) * a.CoutP + co0 + wc); \
    }
#define RC_STORE(buf)                                                                          \
    {                                                                                          \
        _Pragma("unroll") for (int j = 0; j < RC_KC / 2; ++j) sX[buf][gk + 2 * j][gp] = rx[j]; \
        _Pragma("unroll") for (int q = 0; q < WPASS; ++q) *reinterpret_cast<rc_f32x4*>(&sW[buf][q * WROWS + wr][wc]) = rw[q]; \
    }

    rc_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }

    const int nch = a.KP / RC_KC;
    RC_LOAD(0)
    RC_STORE(0)
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) RC_LOAD(ch + 1)
#pragma unroll
        for (int kp = 0; kp < RC_KC / 2; ++kp) {
            const float bx = sX[buf][2 * kp + half][wave * 32 + l31];
            const float a0 = sW[buf][2 * kp + half][l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bx, acc0, 0, 0, 0);
            if (BM == 64) {
                const float a1 = sW[buf][2 * kp + half][(BM == 64 ? 32 : 0) + l31];
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bx, acc1, 0, 0, 0);
            }
        }
        if (ch + 1 < nch) RC_STORE(buf ^ 1)      // the other buffer: every wave passed the barrier behind its last reads of it
        __syncthreads();
    }
#undef RC_LOAD
#undef RC_STORE

    // epilogue: relu(fma(acc, alpha, beta)), NCHW stores into channels c0 .. of a Ctot-channel tensor (lanes 0-31 of a register: 32
    // consecutive pixels of one channel)
    const long long en = n0 + wave * 32 + l31;
    if (en >= a.Ntot) return;
    const long long eb = en / OHW;
    const int epix = (int)(en - eb * OHW);
    float* yb = a.y + (eb * a.Ctot + a.c0) * (long long)OHW + epix;
#pragma unroll
    for (int ct = 0; ct < BM / 32; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co < a.Cout) {
                float v = fma_unpacked(ct ? acc1[r] : acc0[r], a.alpha ? a.alpha[co] : 1.0f, a.beta ? a.beta[co] : 0.0f);
                if (a.relu) v = fmaxf(v, 0.0f);
                yb[(long long)co * OHW] = v;
            }
        }
}

__global__ __launch_bounds__(256) void pack_conv_rect_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int K, int CoutP) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)Cout * K) return;
    const int co = (int)(i / K), k = (int)(i - (long long)co * K);
    wp[(long long)k * CoutP + co] = w[i];
}

__global__ __launch_bounds__(256) void pool3_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W, int mode) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % W), oy = (int)((i / W) % H);
    const float* p = x + (i - (long long)oy * W - ox);      // the plane
    double s = 0.0;
    float m = -INFINITY;
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = oy + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = ox + dx;
            if (ix < 0 || ix >= W) continue;
            const float v = p[(long long)iy * W + ix];
            s += (double)v;
            m = fmaxf(m, v);
            ++cnt;
        }
    }
    y[i] = mode ? m : (float)(s / (double)cnt);
}

__global__ __launch_bounds__(256) void global_avg_kernel(const float* __restrict__ x, float* __restrict__ y, long long NC, int HW) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= NC) return;
    const float* p = x + i * HW;
    double s = 0.0;
    for (int k = 0; k < HW; ++k) s += (double)p[k];
    y[i] = (float)(s / (double)HW);
}

// torch's lerp order, every operation rounded separately (this file is compiled without fp contraction):
// h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11), then 2 v - 1
__global__ __launch_bounds__(256) void inception_prep_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W,
                                                              int normalize, const int* __restrict__ th, const int* __restrict__ tw) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    constexpr int S = INCEPTION_SIZE;
    const int ox = (int)(i % S), oy = (int)((i / S) % S);
    const long long plane = i / ((long long)S * S);
    const float* src = x + plane * H * W;
    const float* r0 = src + (long long)th[oy] * W;
    const float* r1 = src + (long long)th[S + oy] * W;
    const float h0 = __int_as_float(th[2 * S + oy]), h1 = __int_as_float(th[3 * S + oy]);
    const int x0 = tw[ox], x1 = tw[S + ox];
    const float w0 = __int_as_float(tw[2 * S + ox]), w1 = __int_as_float(tw[3 * S + ox]);
    const float top = __fadd_rn(__fmul_rn(w0, r0[x0]), __fmul_rn(w1, r0[x1]));
    const float bot = __fadd_rn(__fmul_rn(w0, r1[x0]), __fmul_rn(w1, r1[x1]));
    float v = __fadd_rn(__fmul_rn(h0, top), __fmul_rn(h1, bot));
    if (normalize) v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f);
    y[i] = v;
}

enum { IOP_CONV, IOP_MAXPOOL_S2, IOP_POOL_AVG, IOP_POOL_MAX, IOP_GAP };
enum { T_IN, T_X0, T_X1, T_T0, T_T1, T_TP, T_B0, T_B1, T_B2, T_B3, T_COUNT };      // T_B3: the caller's block-3 buffer, never workspace

struct Program {
    std::vector<IncLayer> layers;
    std::vector<IncOp> ops;
    long long size[T_COUNT] = {};      // floats per image
    long long offset[T_COUNT] = {}, total = 0;
    int out_c[INCEPTION_BLOCKS] = {}, out_hw[INCEPTION_BLOCKS] = {};

    int H = INCEPTION_SIZE, W = INCEPTION_SIZE, blk = 0;      // the running map of the builder

    void note(int t, long long floats) { size[t] = std::max(size[t], floats); }
    int conv(const std::string& name, int cin, int cout, int kh, int kw, int stride, int ph, int pw, int src, int dst, int c0, int cdst) {
        layers.push_back({name, cin, cout, kh, kw, stride, ph, pw});
        ops.push_back({IOP_CONV, (int)layers.size() - 1, src, dst, c0, cin, cdst, H, W, blk});
        const int OH = (H + 2 * ph - kh) / stride + 1, OW = (W + 2 * pw - kw) / stride + 1;
        note(dst, (long long)cdst * OH * OW);
        return OH;
    }
    void c1(const std::string& n, int cin, int cout, int src, int dst, int c0 = 0, int cdst = 0) { conv(n, cin, cout, 1, 1, 1, 0, 0, src, dst, c0, cdst ? cdst : cout); }
    void c3(const std::string& n, int cin, int cout, int pad, int src, int dst, int c0 = 0, int cdst = 0) { conv(n, cin, cout, 3, 3, 1, pad, pad, src, dst, c0, cdst ? cdst : cout); }
    void c3s2(const std::string& n, int cin, int cout, int src, int dst, int c0, int cdst) { conv(n, cin, cout, 3, 3, 2, 0, 0, src, dst, c0, cdst); }
    void c17(const std::string& n, int cin, int cout, int src, int dst, int c0 = 0, int cdst = 0) { conv(n, cin, cout, 1, 7, 1, 0, 3, src, dst, c0, cdst ? cdst : cout); }
    void c71(const std::string& n, int cin, int cout, int src, int dst, int c0 = 0, int cdst = 0) { conv(n, cin, cout, 7, 1, 1, 3, 0, src, dst, c0, cdst ? cdst : cout); }
    void pool(int kind, int c, int src, int dst, int c0 = 0, int cdst = 0) {
        ops.push_back({kind, -1, src, dst, c0, c, cdst ? cdst : c, H, W, blk});
        const int OH = kind == IOP_MAXPOOL_S2 ? (H - 3) / 2 + 1 : H, OW = kind == IOP_MAXPOOL_S2 ? (W - 3) / 2 + 1 : W;
        note(dst, (long long)(cdst ? cdst : c) * OH * OW);
    }
    void down() { H = (H - 3) / 2 + 1; W = (W - 3) / 2 + 1; }      // behind the ops of a stride-2 stage

    void inception_a(const std::string& p, int cin, int pf, int src, int dst) {      // evaluation/inception.py:216-233
        const int ct = 224 + pf;
        c1(p + ".branch1x1", cin, 64, src, dst, 0, ct);
        c1(p + ".branch5x5_1", cin, 48, src, T_T0);
        conv(p + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2, T_T0, dst, 64, ct);
        c1(p + ".branch3x3dbl_1", cin, 64, src, T_T0);
        c3(p + ".branch3x3dbl_2", 64, 96, 1, T_T0, T_T1);
        c3(p + ".branch3x3dbl_3", 96, 96, 1, T_T1, dst, 128, ct);
        pool(IOP_POOL_AVG, cin, src, T_TP);
        c1(p + ".branch_pool", cin, pf, T_TP, dst, 224, ct);
    }
    void inception_b(const std::string& p, int cin, int src, int dst) {              // torchvision InceptionB
        const int ct = 480 + cin;
        c3s2(p + ".branch3x3", cin, 384, src, dst, 0, ct);
        c1(p + ".branch3x3dbl_1", cin, 64, src, T_T0);
        c3(p + ".branch3x3dbl_2", 64, 96, 1, T_T0, T_T1);
        c3s2(p + ".branch3x3dbl_3", 96, 96, T_T1, dst, 384, ct);
        pool(IOP_MAXPOOL_S2, cin, src, dst, 480, ct);
        down();
    }
    void inception_c(const std::string& p, int cin, int c7, int src, int dst) {      // evaluation/inception.py:241-261
        c1(p + ".branch1x1", cin, 192, src, dst, 0, 768);
        c1(p + ".branch7x7_1", cin, c7, src, T_T0);
        c17(p + ".branch7x7_2", c7, c7, T_T0, T_T1);
        c71(p + ".branch7x7_3", c7, 192, T_T1, dst, 192, 768);
        c1(p + ".branch7x7dbl_1", cin, c7, src, T_T0);
        c71(p + ".branch7x7dbl_2", c7, c7, T_T0, T_T1);
        c17(p + ".branch7x7dbl_3", c7, c7, T_T1, T_T0);
        c71(p + ".branch7x7dbl_4", c7, c7, T_T0, T_T1);
        c17(p + ".branch7x7dbl_5", c7, 192, T_T1, dst, 384, 768);
        pool(IOP_POOL_AVG, cin, src, T_TP);
        c1(p + ".branch_pool", cin, 192, T_TP, dst, 576, 768);
    }
    void inception_d(const std::string& p, int cin, int src, int dst) {              // torchvision InceptionD
        const int ct = 512 + cin;
        c1(p + ".branch3x3_1", cin, 192, src, T_T0);
        c3s2(p + ".branch3x3_2", 192, 320, T_T0, dst, 0, ct);
        c1(p + ".branch7x7x3_1", cin, 192, src, T_T0);
        c17(p + ".branch7x7x3_2", 192, 192, T_T0, T_T1);
        c71(p + ".branch7x7x3_3", 192, 192, T_T1, T_T0);
        c3s2(p + ".branch7x7x3_4", 192, 192, T_T0, dst, 320, ct);
        pool(IOP_MAXPOOL_S2, cin, src, dst, 512, ct);
        down();
    }
    void inception_e(const std::string& p, int cin, int pool_kind, int src, int dst) {      // evaluation/inception.py:269-294, :302-328
        c1(p + ".branch1x1", cin, 320, src, dst, 0, 2048);
        c1(p + ".branch3x3_1", cin, 384, src, T_T0);
        conv(p + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1, T_T0, dst, 320, 2048);
        conv(p + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0, T_T0, dst, 704, 2048);
        c1(p + ".branch3x3dbl_1", cin, 448, src, T_T0);
        c3(p + ".branch3x3dbl_2", 448, 384, 1, T_T0, T_T1);
        conv(p + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1, T_T1, dst, 1088, 2048);
        conv(p + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0, T_T1, dst, 1472, 2048);
        pool(pool_kind, cin, src, T_TP);
        c1(p + ".branch_pool", cin, 192, T_TP, dst, 1856, 2048);
    }

    Program() {
        note(T_IN, 3LL * H * W);
        // block 0 (evaluation/inception.py:84-91)
        H = W = conv("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0, T_IN, T_X0, 0, 32);
        H = W = conv("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0, T_X0, T_X1, 0, 32);
        c3("Conv2d_2b_3x3", 32, 64, 1, T_X1, T_X0);
        pool(IOP_MAXPOOL_S2, 64, T_X0, T_B0);
        down();
        out_c[0] = 64; out_hw[0] = H * W;
        // block 1 (:94-100)
        blk = 1;
        c1("Conv2d_3b_1x1", 64, 80, T_B0, T_X0);
        H = W = conv("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0, T_X0, T_X1, 0, 192);
        pool(IOP_MAXPOOL_S2, 192, T_X1, T_B1);
        down();
        out_c[1] = 192; out_hw[1] = H * W;
        // block 2 (:103-114)
        blk = 2;
        inception_a("Mixed_5b", 192, 32, T_B1, T_X0);
        inception_a("Mixed_5c", 256, 64, T_X0, T_X1);
        inception_a("Mixed_5d", 288, 64, T_X1, T_X0);
        inception_b("Mixed_6a", 288, T_X0, T_X1);
        inception_c("Mixed_6b", 768, 128, T_X1, T_X0);
        inception_c("Mixed_6c", 768, 160, T_X0, T_X1);
        inception_c("Mixed_6d", 768, 160, T_X1, T_X0);
        inception_c("Mixed_6e", 768, 192, T_X0, T_B2);
        out_c[2] = 768; out_hw[2] = H * W;
        // block 3 (:117-124)
        blk = 3;
        inception_d("Mixed_7a", 768, T_B2, T_X0);
        inception_e("Mixed_7b", 1280, IOP_POOL_AVG, T_X0, T_X1);
        inception_e("Mixed_7c", 2048, IOP_POOL_MAX, T_X1, T_X0);
        ops.push_back({IOP_GAP, -1, T_X0, T_B3, 0, 2048, 2048, H, W, blk});
        out_c[3] = 2048; out_hw[3] = 1;
        size[T_B3] = 0;
        for (int t = 0; t < T_COUNT; ++t) { offset[t] = total; total += size[t]; }
    }
};

const Program& program() {
    static const Program p;
    return p;
}

int layer_index(const std::string& name) {
    const auto& L = program().layers;
    for (size_t i = 0; i < L.size(); ++i)
        if (L[i].name == name) return (int)i;
    return -1;
}

}  // namespace

const std::vector<IncLayer>& inception_layers() { return program().layers; }

int conv_rect_kp(int Cin, int kh, int kw) { return round_up(Cin * kh * kw, RC_KC); }
int conv_rect_coutp(int Cout) { return round_up(Cout, 64); }

void conv_rect_table(int Cin, int kh, int kw, std::vector<int>& tab) {
    tab.assign((size_t)conv_rect_kp(Cin, kh, kw), -1);
    int k = 0;
    for (int ci = 0; ci < Cin; ++ci)
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx) tab[k++] = ci << 8 | ky << 4 | kx;
}

int launch_pack_conv_rect(const float* w, float* wp, int Cout, int K, hipStream_t s) {
    const int KP = round_up(K, RC_KC), CoutP = conv_rect_coutp(Cout);
    MCVD_HIP_CHECK(hipMemsetAsync(wp, 0, (size_t)KP * CoutP * sizeof(float), s));
    const long long n = (long long)Cout * K;
    hipLaunchKernelGGL(pack_conv_rect_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, wp, Cout, K, CoutP);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_conv_rect(const float* x, const float* wp, const int* tab, const float* alpha, const float* beta, float* y, int N, int Cin, int H,
                     int W, int Cout, int kh, int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, hipStream_t s) {
    MCVD_REQUIRE(x && wp && tab && y, "conv2d_rect: NULL argument");
    MCVD_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "conv2d_rect: bad shape");
    MCVD_REQUIRE(kh >= 1 && kh <= 15 && kw >= 1 && kw <= 15 && stride >= 1 && ph >= 0 && pw >= 0,
                 "conv2d_rect: kernel %d x %d (1 to 15 each), stride %d, padding (%d, %d)", kh, kw, stride, ph, pw);
    MCVD_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "conv2d_rect: the %d x %d kernel exceeds the padded %d x %d input", kh, kw, H, W);
    MCVD_REQUIRE(c0 >= 0 && c0 + Cout <= Ctot, "conv2d_rect: channels [%d, %d) do not fit the %d-channel output", c0, c0 + Cout, Ctot);
    ConvRectArgs a;
    a.x = x; a.wp = wp; a.tab = tab; a.alpha = alpha; a.beta = beta; a.y = y;
    a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.CoutP = conv_rect_coutp(Cout); a.stride = stride; a.ph = ph; a.pw = pw;
    a.OH = (H + 2 * ph - kh) / stride + 1;
    a.OW = (W + 2 * pw - kw) / stride + 1;
    a.K = Cin * kh * kw; a.KP = conv_rect_kp(Cin, kh, kw); a.relu = relu; a.c0 = c0; a.Ctot = Ctot;
    a.Ntot = (long long)N * a.OH * a.OW;
    MCVD_REQUIRE((long long)Cin * H * W < (1LL << 31) && (long long)Cin * kh * kw < (1LL << 23), "conv2d_rect: an image exceeds 32-bit offsets");
    MCVD_REQUIRE((long long)Ctot * a.OH * a.OW < (1LL << 31), "conv2d_rect: an output image exceeds 32-bit offsets");
    const long long tiles = (a.Ntot + RC_BN - 1) / RC_BN;
    MCVD_REQUIRE(tiles < (1LL << 31) && a.CoutP / 32 < 65536, "conv2d_rect: %lld pixel tiles exceed one launch", tiles);
    const bool one = kh == 1 && kw == 1 && stride == 1 && ph == 0 && pw == 0;
    const int BM = Cout <= 32 ? 32 : 64;
    const dim3 grid((unsigned)tiles, (unsigned)ceil_div(Cout, BM));
    if (BM == 32 && one) hipLaunchKernelGGL((conv_rect_mfma_kernel<32, true>), grid, dim3(RC_THREADS), 0, s, a);
    else if (BM == 32) hipLaunchKernelGGL((conv_rect_mfma_kernel<32, false>), grid, dim3(RC_THREADS), 0, s, a);
    else if (one) hipLaunchKernelGGL((conv_rect_mfma_kernel<64, true>), grid, dim3(RC_THREADS), 0, s, a);
    else hipLaunchKernelGGL((conv_rect_mfma_kernel<64, false>), grid, dim3(RC_THREADS), 0, s, a);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_pool3(const float* x, float* y, long long NC, int H, int W, int mode, hipStream_t s) {
    MCVD_REQUIRE(x && y && NC > 0 && H > 0 && W > 0, "pool3: bad arguments");
    MCVD_REQUIRE(mode == 0 || mode == 1, "pool3: mode %d (0 = average without the padding, 1 = max)", mode);
    const long long total = NC * H * W, blocks = (total + 255) / 256;
    MCVD_REQUIRE(blocks < (1LL << 31), "pool3: %lld workgroups exceed one launch", blocks);
    hipLaunchKernelGGL(pool3_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, total, H, W, mode);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_global_avg(const float* x, float* y, long long NC, int HW, hipStream_t s) {
    MCVD_REQUIRE(x && y && NC > 0 && HW > 0, "global_avg: bad arguments");
    const long long blocks = (NC + 255) / 256;
    MCVD_REQUIRE(blocks < (1LL << 31), "global_avg: %lld workgroups exceed one launch", blocks);
    hipLaunchKernelGGL(global_avg_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, NC, HW);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

void inception_axis_table(int S, std::vector<int>& tab) {
    constexpr int O = INCEPTION_SIZE;
    tab.assign(4 * O, 0);
    const float scale = (float)S / (float)O;                       // area_pixel_compute_scale: fl32(S / 299)
    for (int dpos = 0; dpos < O; ++dpos) {
        // scale * (d + 0.5) is exact in double (24 x 10 bits) and so is the subtraction: ONE rounding, the fused multiply-subtract's value
        float src = (float)((double)scale * ((double)dpos + 0.5) - 0.5);
        if (src < 0.0f) src = 0.0f;
        int a = (int)src;                                          // floor: src >= 0
        if (a > S - 1) a = S - 1;
        const float lam = src - (float)a;
        const float l0 = 1.0f - lam;
        tab[dpos] = a;
        tab[O + dpos] = a + 1 < S ? a + 1 : S - 1;
        memcpy(&tab[2 * O + dpos], &l0, sizeof(float));
        memcpy(&tab[3 * O + dpos], &lam, sizeof(float));
    }
}

int launch_inception_prep(const float* x, float* y, long long n, int H, int W, int normalize, const int* tab_h, const int* tab_w, hipStream_t s) {
    MCVD_REQUIRE(x && y && tab_h && tab_w && n > 0 && H > 0 && W > 0, "inception_prep: bad arguments");
    MCVD_REQUIRE((long long)H * W < (1LL << 31), "inception_prep: a %d x %d plane exceeds 32-bit offsets", H, W);
    const long long total = n * 3 * INCEPTION_SIZE * INCEPTION_SIZE, blocks = (total + 255) / 256;
    MCVD_REQUIRE(blocks < (1LL << 31), "inception_prep: %lld workgroups exceed one launch", blocks);
    hipLaunchKernelGGL(inception_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, total, H, W, normalize, tab_h, tab_w);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ the net
int inception_set_param(mcvd_inception* n, const char* name, const float* host, int64_t numel) {
    static const char* const SUFFIX[5] = {".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"};
    const std::string full(name);
    for (int k = 0; k < 5; ++k) {
        const size_t sl = strlen(SUFFIX[k]);
        if (full.size() <= sl || full.compare(full.size() - sl, sl, SUFFIX[k])) continue;
        const int li = layer_index(full.substr(0, full.size() - sl));
        if (li < 0) break;
        const IncLayer& L = program().layers[li];
        const int64_t want = k == 0 ? (int64_t)L.Cout * L.Cin * L.kh * L.kw : L.Cout;
        MCVD_REQUIRE(numel == want, "inception_set_param: '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)want);
        std::vector<float>& dst = (k == 0 ? n->w : k == 1 ? n->bn_w : k == 2 ? n->bn_b : k == 3 ? n->bn_m : n->bn_v)[li];
        dst.assign(host, host + numel);
        n->finalized = false;
        return 0;
    }
    MCVD_REQUIRE(false, "inception_set_param: unknown parameter '%s'", name);
    return 0;
}

int inception_finalize(mcvd_inception* n) {
    hipStream_t s = n->ctx->stream;
    const std::vector<IncLayer>& LS = program().layers;
    const int NL = (int)LS.size();
    for (int i = 0; i < NL; ++i) {
        const char* missing = n->w[i].empty() ? ".conv.weight" : n->bn_w[i].empty() ? ".bn.weight" : n->bn_b[i].empty() ? ".bn.bias"
                              : n->bn_m[i].empty() ? ".bn.running_mean" : n->bn_v[i].empty() ? ".bn.running_var" : nullptr;
        if (missing) { set_error("inception_finalize: missing %s%s", LS[i].name.c_str(), missing); return MCVD_ESTATE; }
    }
    size_t total = 0, raw_max = 0;
    for (int i = 0; i < NL; ++i) {
        const IncLayer& L = LS[i];
        total += (size_t)conv_rect_kp(L.Cin, L.kh, L.kw) * (conv_rect_coutp(L.Cout) + 1) + 2 * (size_t)round_up(L.Cout, 4);
        raw_max = std::max(raw_max, n->w[i].size());
    }
    MCVD_HIP_CHECK(hipStreamSynchronize(s));
    if (n->params) MCVD_HIP_CHECK(hipFree(n->params));
    n->params = nullptr;
    MCVD_HIP_CHECK(hipMalloc((void**)&n->params, total * sizeof(float)));
    float* raw = nullptr;
    MCVD_HIP_CHECK(hipMalloc((void**)&raw, raw_max * sizeof(float)));
    float* o = n->params;
    int rc = 0;
    std::vector<float> al, be;
    std::vector<int> tab;
    for (int i = 0; i < NL && !rc; ++i) {
        const IncLayer& L = LS[i];
        const int KP = conv_rect_kp(L.Cin, L.kh, L.kw);
        n->wp[i] = o; o += (size_t)KP * conv_rect_coutp(L.Cout);
        n->alpha[i] = o; o += round_up(L.Cout, 4);
        n->beta[i] = o; o += round_up(L.Cout, 4);
        n->tab[i] = reinterpret_cast<int*>(o); o += KP;
        al.resize(L.Cout);
        be.resize(L.Cout);
        for (int c = 0; c < L.Cout; ++c) {      // fp64, rounded once each
            const double a64 = (double)n->bn_w[i][c] / sqrt((double)n->bn_v[i][c] + 0.001);
            al[c] = (float)a64;
            be[c] = (float)((double)n->bn_b[i][c] - (double)n->bn_m[i][c] * a64);
        }
        conv_rect_table(L.Cin, L.kh, L.kw, tab);
        hipError_t e = hipMemcpyAsync(raw, n->w[i].data(), n->w[i].size() * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n->alpha[i], al.data(), (size_t)L.Cout * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n->beta[i], be.data(), (size_t)L.Cout * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n->tab[i], tab.data(), (size_t)KP * sizeof(int), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { set_error("inception_finalize: upload failed: %s", hipGetErrorString(e)); rc = MCVD_EHIP; break; }
        rc = launch_pack_conv_rect(raw, n->wp[i], L.Cout, L.Cin * L.kh * L.kw, s);
        if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("inception_finalize: synchronize failed"); rc = MCVD_EHIP; }      // `raw`, `al`, `be`, `tab` are reused
    }
    (void)hipFree(raw);
    if (rc) return rc;
    n->finalized = true;
    return 0;
}

static int axis_tab(mcvd_inception* n, int in_size, const int** tab) {
    auto it = n->axis.find(in_size);
    if (it == n->axis.end()) {
        std::vector<int> host;
        inception_axis_table(in_size, host);
        int* dev = nullptr;
        MCVD_HIP_CHECK(hipMalloc((void**)&dev, host.size() * sizeof(int)));
        MCVD_HIP_CHECK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, n->ctx->stream));
        MCVD_HIP_CHECK(hipStreamSynchronize(n->ctx->stream));      // `host` goes out of scope
        it = n->axis.emplace(in_size, dev).first;
    }
    *tab = it->second;
    return 0;
}

int inception_forward(mcvd_inception* n, const float* images01, int64_t count, int H, int W, int resize_input, int normalize_input,
                      int block_mask, float* const* out) {
    hipStream_t s = n->ctx->stream;
    const Program& P = program();
    MCVD_REQUIRE(resize_input || (H == INCEPTION_SIZE && W == INCEPTION_SIZE), "inception_forward: without resize_input the images must be 299 x 299, got %d x %d", H, W);
    int last = -1;
    for (int b = 0; b < INCEPTION_BLOCKS; ++b)
        if (block_mask >> b & 1) {
            MCVD_REQUIRE(out[b], "inception_forward: block %d is requested and its output is NULL", b);
            last = b;
        }
    MCVD_REQUIRE(last >= 0 && !(block_mask >> INCEPTION_BLOCKS), "inception_forward: block_mask 0x%x (bits 0 to 3, at least one)", block_mask);
    const int cap = (int)std::min<int64_t>(count, INCEPTION_CHUNK);
    if (n->ws_images < cap) {
        MCVD_HIP_CHECK(hipStreamSynchronize(s));
        if (n->ws) MCVD_HIP_CHECK(hipFree(n->ws));
        n->ws = nullptr;
        n->ws_images = 0;
        MCVD_HIP_CHECK(hipMalloc((void**)&n->ws, (size_t)P.total * cap * sizeof(float)));
        n->ws_images = cap;
    }
    const int *tab_h, *tab_w;
    if (int rc = axis_tab(n, H, &tab_h)) return rc;
    if (int rc = axis_tab(n, W, &tab_w)) return rc;
    const long long wcap = n->ws_images;

    for (int64_t f0 = 0; f0 < count; f0 += cap) {
        const int nimg = (int)std::min<int64_t>(cap, count - f0);
        auto ptr = [&](int t) -> float* {
            if (t >= T_B0 && (block_mask >> (t - T_B0) & 1)) return out[t - T_B0] + f0 * P.out_c[t - T_B0] * P.out_hw[t - T_B0];
            return n->ws + P.offset[t] * wcap;
        };
        if (int rc = launch_inception_prep(images01 + f0 * 3 * H * W, ptr(T_IN), nimg, H, W, normalize_input, tab_h, tab_w, s)) return rc;
        for (const IncOp& op : P.ops) {
            if (op.block > last) break;
            const float* x = ptr(op.src);
            float* y = ptr(op.dst);
            int rc = 0;
            if (op.kind == IOP_CONV) {
                const IncLayer& L = P.layers[op.layer];
                rc = launch_conv_rect(x, n->wp[op.layer], n->tab[op.layer], n->alpha[op.layer], n->beta[op.layer], y, nimg, L.Cin, op.H, op.W, L.Cout,
                                      L.kh, L.kw, L.stride, L.ph, L.pw, 1, op.c0, op.Cdst, s);
            } else if (op.kind == IOP_MAXPOOL_S2) {
                const int OH = (op.H - 3) / 2 + 1, OW = (op.W - 3) / 2 + 1;
                if (op.Cdst == op.Csrc) {
                    rc = launch_maxpool3s2(x, y, (long long)nimg * op.Csrc, op.H, op.W, s);
                } else {      // a channel slice of the block's output: the images' slices are not contiguous, one launch per image
                    for (int i = 0; i < nimg && !rc; ++i)
                        rc = launch_maxpool3s2(x + (long long)i * op.Csrc * op.H * op.W, y + ((long long)i * op.Cdst + op.c0) * OH * OW, op.Csrc, op.H,
                                               op.W, s);
                }
            } else if (op.kind == IOP_POOL_AVG || op.kind == IOP_POOL_MAX) {
                rc = launch_pool3(x, y, (long long)nimg * op.Csrc, op.H, op.W, op.kind == IOP_POOL_MAX, s);
            } else {
                rc = launch_global_avg(x, y, (long long)nimg * op.Csrc, op.H * op.W, s);
            }
            if (rc) return rc;
        }
    }
    return 0;
}

}  // namespace mcvd

mcvd_inception::mcvd_inception() {
    const size_t nl = mcvd::inception_layers().size();
    w.resize(nl); bn_w.resize(nl); bn_b.resize(nl); bn_m.resize(nl); bn_v.resize(nl);
    wp.assign(nl, nullptr); alpha.assign(nl, nullptr); beta.assign(nl, nullptr); tab.assign(nl, nullptr);
}

mcvd_inception::~mcvd_inception() {
    if (params) (void)hipFree(params);
    if (ws) (void)hipFree(ws);
    for (auto& kv : axis) (void)hipFree(kv.second);
}
