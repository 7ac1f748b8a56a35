// The kernels and the host scaffold that the detector nets share (detector_ops.h): LPIPS's AlexNet stack (lpips.cpp) and the FID
// InceptionV3 (inception.cpp) run every conv on conv_mfma_kernel and their pools on the three pool kernels below.
//
// conv_mfma_kernel: D[co][n] = sum_k Wp[k][co] X[k][n] on v_mfma_f32_32x32x2_f32.  A operand = weights (rows = output channels), B operand
// = the im2col of the input, gathered on the fly (k = (ci * kh + ky) * kw + kx; n = image * OH * OW + oy * OW + ox), so an accumulator
// register holds 32 consecutive output pixels of one channel across lanes and the NCHW stores are contiguous runs; 7 x 7 and 8 x 8 maps
// fill tiles across the batch.  Exact fp32 products, per output ONE fma chain in the fixed order k = 0 .. K-1 (lanes 0-31 feed row 2 kp,
// lanes 32-63 row 2 kp + 1 of every MFMA), so a result does not depend on the tile, on the other images of the batch or on the chunking;
// padding rows are zero weights against zero inputs.  Workgroup = 4 wave64 = BM output channels x 128 pixels (BM = 64, or 32 for layers
// of at most 32 output channels, which would otherwise run half their MFMAs on padding), K in chunks of 32 rows, double-buffered in LDS
// (2 x 32 x (BM + 128) floats: 48 KB) with a register prefetch of chunk i + 1 under the MFMAs of chunk i: one barrier per chunk.
// k -> (ci, ky, kx) comes from a per-layer table built on the host (one scalar load per k row, no div / mod in the gather); a 1 x 1 layer
// (stride 1, no padding) takes the path whose B operand is the plain strided load x[k][pixel].
// Why 32 rows: where a launch has fewer workgroups than the device has compute units (InceptionV3's 17 x 17 and 8 x 8 maps, AlexNet's
// 7 x 7) a workgroup runs alone and a K chunk costs one load latency whatever its depth, so 32 rows halve the number of such waits against
// 16.  AlexNet's two large-grid layers could hold twice the workgroups with 24 KB of LDS; a frame_lpips call as a whole is not slower at
// 32 rows than at 16 (profiles/lpips_time.txt: whole-call medians, no per-layer figures).
// Everything runs on the caller's stream; nothing reads the environment.
#include "../detector_ops.h"

#include "mcvd_hip.h"

#include <math.h>
#include <string.h>

namespace mcvd {
namespace {

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));
typedef float cv_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CV_BN = 128, CV_KC = 32, CV_THREADS = 256, CV_COUTP = 64, CV_TAP_BITS = 5;

struct DetConvArgs {
    const float* x;
    const float* wp;
    const int* tab;         // [KP]: ci << 10 | ky << 5 | kx, -1 beyond K
    const float* alpha;     // [Cout] or null (1)
    const float* beta;      // [Cout] or null (0)
    float* y;
    int Cin, H, W, Cout, CoutP, stride, ph, pw, OH, OW, K, KP, relu, c0, Ctot;
    long long Ntot;         // images * OH * OW
};

template <int BM, bool ONE>
__global__ __launch_bounds__(CV_THREADS) void conv_mfma_kernel(DetConvArgs a) {
    __shared__ __attribute__((aligned(16))) float sW[2][CV_KC][BM];
    __shared__ float sX[2][CV_KC][CV_BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long n0 = (long long)blockIdx.x * CV_BN;
    const int co0 = blockIdx.y * BM;
    const int OHW = a.OH * a.OW, HW = a.H * a.W;

    // gather role: this thread stages pixel gp of the tile for the k rows gk, gk + 2, ..., gk + 30 of every chunk (gk is wave-uniform)
    const int gp = tid & (CV_BN - 1), gk = __builtin_amdgcn_readfirstlane(tid >> 7);
    const long long gn = n0 + gp;
    const bool gvalid = gn < a.Ntot;
    const long long gb = gvalid ? gn / OHW : 0;
    const int gpix = gvalid ? (int)(gn - gb * OHW) : 0;
    const int goy = gpix / a.OW, gox = gpix - goy * a.OW;
    const int iy0 = goy * a.stride - a.ph, ix0 = gox * a.stride - a.pw;
    const float* xb = a.x + gb * (long long)a.Cin * HW;
    // weight role: rows wr, wr + WROWS, ... of the chunk, columns wc .. wc + 3 (BM = 64: 16 rows per pass, two passes; BM = 32: one pass)
    constexpr int WQ = BM / 4, WROWS = CV_THREADS / WQ, WPASS = CV_KC / WROWS;
    static_assert(WPASS >= 1 && WPASS * WROWS == CV_KC, "the weight role must cover the chunk");
    const int wr = tid / WQ, wc = (tid % WQ) * 4;

    float rx[CV_KC / 2];
    cv_f32x4 rw[WPASS];
    // loads are unconditional (a dead element reads the image's first value and is discarded): no branch around a load
#define CV_LOAD(ch)                                                                                                  \
    {                                                                                                                \
        _Pragma("unroll") for (int j = 0; j < CV_KC / 2; ++j) {                                                         \
            const int k = (ch) * CV_KC + gk + 2 * j;                                                                    \
            bool ok;                                                                                                 \
            int off;                                                                                                 \
            if (ONE) {                                                                                               \
                ok = gvalid && k < a.K;                                                                              \
                off = k * HW + gpix;                                                                                 \
            } else {                                                                                                 \
                const int t = a.tab[k];                                                                              \
                const int iy = iy0 + ((t >> CV_TAP_BITS) & 31), ix = ix0 + (t & 31);                                 \
                ok = gvalid && t >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;                                 \
                off = (t >> 2 * CV_TAP_BITS) * HW + iy * a.W + ix;                                                   \
            }                                                                                                        \
            const float v = xb[ok ? off : 0];                                                                        \
            rx[j] = ok ? v : 0.0f;                                                                                   \
        }                                                                                                            \
        _Pragma("unroll") for (int q = 0; q < WPASS; ++q)                                                            \
            rw[q] = *reinterpret_cast<const cv_f32x4*>(a.wp + (long long)((ch) * CV_KC + q * WROWS + wr) * a.CoutP + co0 + wc); \
    }
#define CV_STORE(buf)                                                                          \
    {                                                                                          \
        _Pragma("unroll") for (int j = 0; j < CV_KC / 2; ++j) sX[buf][gk + 2 * j][gp] = rx[j];    \
        _Pragma("unroll") for (int q = 0; q < WPASS; ++q) *reinterpret_cast<cv_f32x4*>(&sW[buf][q * WROWS + wr][wc]) = rw[q]; \
    }

    cv_f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }

    const int nch = a.KP / CV_KC;
    CV_LOAD(0)
    CV_STORE(0)
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) CV_LOAD(ch + 1)
#pragma unroll
        for (int kp = 0; kp < CV_KC / 2; ++kp) {
            const float bx = sX[buf][2 * kp + half][wave * 32 + l31];
            const float a0 = sW[buf][2 * kp + half][l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bx, acc0, 0, 0, 0);
            if (BM == 64) {
                const float a1 = sW[buf][2 * kp + half][(BM == 64 ? 32 : 0) + l31];
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bx, acc1, 0, 0, 0);
            }
        }
        if (ch + 1 < nch) CV_STORE(buf ^ 1)      // the other buffer: every wave passed the barrier behind its last reads of it
        __syncthreads();
    }
#undef CV_LOAD
#undef CV_STORE

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

__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int K, int CoutP) {
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

}  // namespace

int conv_kp(int Cin, int kh, int kw) { return round_up(Cin * kh * kw, CV_KC); }
int conv_coutp(int Cout) { return round_up(Cout, CV_COUTP); }

void conv_table(int Cin, int kh, int kw, std::vector<int>& tab) {
    tab.assign((size_t)conv_kp(Cin, kh, kw), -1);
    int k = 0;
    for (int ci = 0; ci < Cin; ++ci)
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx) tab[k++] = ci << 2 * CV_TAP_BITS | ky << CV_TAP_BITS | kx;
}

int launch_pack_conv(const float* w, float* wp, int Cout, int K, hipStream_t s) {
    const int KP = round_up(K, CV_KC), CoutP = conv_coutp(Cout);
    MCVD_HIP_CHECK(hipMemsetAsync(wp, 0, (size_t)KP * CoutP * sizeof(float), s));
    const long long n = (long long)Cout * K;
    hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, wp, Cout, K, CoutP);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_conv(const float* x, const float* wp, const int* tab, const float* alpha, const float* beta, float* y, int N, int Cin, int H, int W,
                int Cout, int kh, int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, const char* who, hipStream_t s) {
    MCVD_REQUIRE(x && wp && tab && y, "%s: NULL argument", who);
    MCVD_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad shape", who);
    MCVD_REQUIRE(kh >= 1 && kh <= 31 && kw >= 1 && kw <= 31 && stride >= 1 && ph >= 0 && pw >= 0,
                 "%s: kernel %d x %d (1 to 31 each), stride %d, padding (%d, %d)", who, kh, kw, stride, ph, pw);
    MCVD_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: the %d x %d kernel exceeds the padded %d x %d input", who, kh, kw, H, W);
    MCVD_REQUIRE(c0 >= 0 && c0 + Cout <= Ctot, "%s: channels [%d, %d) do not fit the %d-channel output", who, c0, c0 + Cout, Ctot);
    DetConvArgs a;
    a.x = x; a.wp = wp; a.tab = tab; a.alpha = alpha; a.beta = beta; a.y = y;
    a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.CoutP = conv_coutp(Cout); a.stride = stride; a.ph = ph; a.pw = pw;
    a.OH = (H + 2 * ph - kh) / stride + 1;
    a.OW = (W + 2 * pw - kw) / stride + 1;
    a.K = Cin * kh * kw; a.KP = conv_kp(Cin, kh, kw); a.relu = relu; a.c0 = c0; a.Ctot = Ctot;
    a.Ntot = (long long)N * a.OH * a.OW;
    // ci sits above the two 5-bit taps of a table entry, which stays a non-negative int
    MCVD_REQUIRE((long long)Cin * H * W < (1LL << 31) && Cin < (1 << (31 - 2 * CV_TAP_BITS)) && (long long)Cin * kh * kw < (1LL << 30),
                 "%s: an image exceeds 32-bit offsets", who);
    MCVD_REQUIRE((long long)a.OH * a.OW < (1LL << 31), "%s: an output map exceeds 32-bit offsets", who);      // the kernel's output offsets are 64-bit
    const long long tiles = (a.Ntot + CV_BN - 1) / CV_BN;
    MCVD_REQUIRE(tiles < (1LL << 31) && a.CoutP / 32 < 65536, "%s: %lld pixel tiles exceed one launch", who, tiles);
    const bool one = kh == 1 && kw == 1 && stride == 1 && ph == 0 && pw == 0;
    const int BM = Cout <= 32 ? 32 : 64;
    const dim3 grid((unsigned)tiles, (unsigned)ceil_div(Cout, BM));
    if (BM == 32 && one) hipLaunchKernelGGL((conv_mfma_kernel<32, true>), grid, dim3(CV_THREADS), 0, s, a);
    else if (BM == 32) hipLaunchKernelGGL((conv_mfma_kernel<32, false>), grid, dim3(CV_THREADS), 0, s, a);
    else if (one) hipLaunchKernelGGL((conv_mfma_kernel<64, true>), grid, dim3(CV_THREADS), 0, s, a);
    else hipLaunchKernelGGL((conv_mfma_kernel<64, false>), grid, dim3(CV_THREADS), 0, s, a);
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

// ------------------------------------------------------------------ a net's parameters
ParamBlob::~ParamBlob() {
    if (raw) (void)hipFree(raw);
}

size_t ParamBlob::floats_needed(const ConvGeom& g) {      // packed weights, the table, alpha and beta
    return (size_t)conv_kp(g.Cin, g.kh, g.kw) * (conv_coutp(g.Cout) + 1) + 2 * (size_t)round_up(g.Cout, 4);
}

int ParamBlob::begin(float** params, size_t floats, size_t raw_floats) {
    size_t none = 0;      // a new blob every time
    if (int rc = grow(reinterpret_cast<void**>(params), &none, floats * sizeof(float), s)) return rc;
    MCVD_HIP_CHECK(hipMalloc((void**)&raw, raw_floats * sizeof(float)));
    cursor = *params;
    return 0;
}

float* ParamBlob::take(int n) {
    float* p = cursor;
    cursor += round_up(n, 4);
    return p;
}

int ParamBlob::conv(const ConvGeom& g, const float* w, const float* alpha, const float* beta, ConvParams* out) {
    const int K = g.Cin * g.kh * g.kw, KP = conv_kp(g.Cin, g.kh, g.kw);
    std::vector<int> tab;
    conv_table(g.Cin, g.kh, g.kw, tab);
    out->wp = cursor; cursor += (size_t)KP * conv_coutp(g.Cout);
    float* const al = take(g.Cout);
    float* const be = take(g.Cout);
    out->alpha = alpha ? al : nullptr;
    out->beta = beta ? be : nullptr;
    out->tab = reinterpret_cast<int*>(cursor); cursor += KP;
    hipError_t e = hipMemcpyAsync(raw, w, (size_t)g.Cout * K * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && alpha) e = hipMemcpyAsync(out->alpha, alpha, (size_t)g.Cout * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && beta) e = hipMemcpyAsync(out->beta, beta, (size_t)g.Cout * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out->tab, tab.data(), (size_t)KP * sizeof(int), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { set_error("%s: upload failed: %s", who, hipGetErrorString(e)); return MCVD_EHIP; }
    if (int rc = launch_pack_conv(raw, out->wp, g.Cout, K, s)) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) { set_error("%s: synchronize failed", who); return MCVD_EHIP; }      // `raw`, `tab` and the caller's vectors are reused
    return 0;
}

// ------------------------------------------------------------------ a net's workspaces and tables
int grow(void** ptr, size_t* have, size_t need, hipStream_t s) {
    if (*have >= need && *ptr) return 0;
    MCVD_HIP_CHECK(hipStreamSynchronize(s));
    if (*ptr) MCVD_HIP_CHECK(hipFree(*ptr));
    *ptr = nullptr;
    *have = 0;
    MCVD_HIP_CHECK(hipMalloc(ptr, need));
    *have = need;
    return 0;
}

TableCache::~TableCache() {
    for (auto& kv : map) (void)hipFree(kv.second.dev);
}

int TableCache::get(int size, int (*build)(int size, std::vector<int>& host), hipStream_t s, const Entry** out) {
    auto it = map.find(size);
    if (it == map.end()) {
        std::vector<int> host;
        const int aux = build(size, host);
        int* dev = nullptr;
        MCVD_HIP_CHECK(hipMalloc((void**)&dev, host.size() * sizeof(int)));
        MCVD_HIP_CHECK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
        MCVD_HIP_CHECK(hipStreamSynchronize(s));      // `host` goes out of scope
        it = map.emplace(size, Entry{dev, aux}).first;
    }
    *out = &it->second;
    return 0;
}

void bilinear_axis_table(int S, int O, int* i0, int* i1, float* l0, float* l1) {
    const float scale = (float)S / (float)O;                       // area_pixel_compute_scale: fl32(S / O)
    for (int dpos = 0; dpos < O; ++dpos) {
        // scale * (d + 0.5) is exact in double (24 bits x the few of d + 0.5) and so is the subtraction: ONE rounding, the fused
        // multiply-subtract's value
        float src = (float)((double)scale * ((double)dpos + 0.5) - 0.5);
        if (src < 0.0f) src = 0.0f;
        int a = (int)src;                                          // floor: src >= 0
        if (a > S - 1) a = S - 1;
        const float lam = src - (float)a;
        i0[dpos] = a;
        i1[dpos] = a + 1 < S ? a + 1 : S - 1;
        l0[dpos] = 1.0f - lam;
        l1[dpos] = lam;
    }
}

}  // namespace mcvd
