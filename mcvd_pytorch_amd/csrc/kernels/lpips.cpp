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
// Kernels: lpips_prep_h / lpips_prep_v (quantise + resize + normalise), lpips_distance_kernel (one workgroup per frame and tap, fp64 sums
// in a fixed order: bit-identical run to run).  The five convs (bias + ReLU in the epilogue) and the two pools are the detector nets'
// shared ones (detector_ops.h, kernels/detector_ops.cpp: conv_mfma_kernel, maxpool3s2_kernel).  Everything runs on the context's stream;
// nothing reads the environment.
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
// in the same order in double (this file is compiled without fp contraction).  Layout as the prep kernels read it; returns the taps per
// output position.
int resize_table(int in_size, std::vector<int>& tab) {
    const int out_size = LPIPS_SIZE;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    tab.assign((size_t)2 * out_size + (size_t)out_size * ksize, 0);
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
    return ksize;
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

// ------------------------------------------------------------------ the net
static ConvGeom geom(int k) { return {LPIPS_LAYERS[k].Cin, LPIPS_LAYERS[k].Cout, LPIPS_LAYERS[k].ks, LPIPS_LAYERS[k].ks}; }

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
        total += ParamBlob::floats_needed(geom(k)) + (size_t)round_up(LPIPS_LAYERS[k].Cout, 4);
        raw_max = std::max(raw_max, n->w[k].size());
    }
    ParamBlob blob(n->ctx->stream, "lpips_finalize");
    if (int rc = blob.begin(&n->params, total, raw_max)) return rc;
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        n->lind[k] = blob.take(LPIPS_LAYERS[k].Cout);
        MCVD_HIP_CHECK(hipMemcpyAsync(n->lind[k], n->lin[k].data(), n->lin[k].size() * sizeof(float), hipMemcpyHostToDevice, blob.s));
        if (int rc = blob.conv(geom(k), n->w[k].data(), nullptr, n->b[k].data(), &n->conv[k])) return rc;
    }
    for (int c = 0; c < 3; ++c) { n->sh[c] = n->shift[c]; n->sc[c] = n->scale[c]; }
    n->finalized = true;
    return 0;
}

static int resize_tab(mcvd_lpips* n, int in_size, const int** tab, int* ksize) {
    *tab = nullptr;
    *ksize = 0;
    if (in_size == LPIPS_SIZE) return 0;      // Pillow skips a pass whose input and output length agree
    const TableCache::Entry* e;
    if (int rc = n->tabs.get(in_size, resize_table, n->ctx->stream, &e)) return rc;
    *tab = e->dev;
    *ksize = e->aux;
    return 0;
}

int lpips_frames(mcvd_lpips* n, const float* pred01, const float* real01, int B, int T, int C, int H, int W, float* lpips_out,
                 unsigned char* resized_out, float* per_tap_out) {
    hipStream_t s = n->ctx->stream;
    const long long nfr = (long long)B * T;
    const int cap = (int)std::min<long long>(nfr, LPIPS_CHUNK);
    const WsLayout lay(cap);      // a workspace left larger by an earlier call holds it as well
    if (int rc = grow((void**)&n->ws, &n->ws_bytes, (size_t)lay.total * sizeof(float), s)) return rc;
    const size_t rows_need = (size_t)cap * 2 * C * H * LPIPS_SIZE;
    if (int rc = grow((void**)&n->rows, &n->rows_bytes, rows_need, s)) return rc;
    const int *tab_w, *tab_h;
    int ks_w, ks_h;
    if (int rc = resize_tab(n, W, &tab_w, &ks_w)) return rc;
    if (int rc = resize_tab(n, H, &tab_h, &ks_h)) return rc;
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
            const ConvParams& cv = n->conv[k];
            if (int rc = launch_conv(x, cv.wp, cv.tab, nullptr, cv.beta, y, (int)nimg, L.Cin, L.H, L.H, L.Cout, L.ks, L.ks, L.stride, L.pad, L.pad, 1, 0,
                                     L.Cout, "lpips_frames", s))
                return rc;
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
}
