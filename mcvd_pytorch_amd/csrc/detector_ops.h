// What the detector nets (LPIPS's AlexNet stack, kernels/lpips.cpp; the FID InceptionV3, kernels/inception.cpp) are made of and share
// (kernels/detector_ops.cpp): the one general conv, the pools, and the host-side scaffold of a net -- its parameter blob, its workspaces,
// its per-size tables.
#pragma once
#include <map>
#include <vector>

#include "common.h"

namespace mcvd {

// ------------------------------------------------------------------ the conv
// Any kernel size up to 31 x 31, stride and zero padding as an implicit GEMM on v_mfma_f32_32x32x2_f32, pixels of all images flattened
// into the GEMM's N; the epilogue is y[:, c0 + co] = relu?(fma(acc, alpha[co], beta[co])) into a tensor of Ctot channels (alpha null: 1,
// beta null: 0, so a conv with a bias is alpha = null, beta = bias: fma(acc, 1, b) is acc + b rounded once).  Packed weights:
// wp[k * CoutP + co], k = (ci * kh + ky) * kw + kx, K padded to a multiple of 32 and Cout to one of 64, zeros.
// tab[k] = ci << 10 | ky << 5 | kx, -1 for k >= K.  `who` names the caller's entry point in the error messages.
int conv_kp(int Cin, int kh, int kw);
int conv_coutp(int Cout);
void conv_table(int Cin, int kh, int kw, std::vector<int>& tab);                      // conv_kp entries
int launch_pack_conv(const float* w, float* wp, int Cout, int K, hipStream_t s);      // wp: conv_kp * conv_coutp floats
int launch_conv(const float* x, const float* wp, const int* tab, const float* alpha, const float* beta, float* y, int N, int Cin, int H, int W,
                int Cout, int kh, int kw, int stride, int ph, int pw, int relu, int c0, int Ctot, const char* who, hipStream_t s);

// ------------------------------------------------------------------ the pools
// MaxPool2d(3, 2) over [NC, H, W] planes
int launch_maxpool3s2(const float* x, float* y, long long NC, int H, int W, hipStream_t s);
// 3 x 3, stride 1, padding 1 over [NC, H, W] planes.  mode 0: F.avg_pool2d(count_include_pad=False) (fp64 sum in window order, divided by
// the 4 / 6 / 9 values inside the map, rounded once); mode 1: F.max_pool2d.
int launch_pool3(const float* x, float* y, long long NC, int H, int W, int mode, hipStream_t s);
// y[i] = (float)(sum of x[i][0 .. HW) in fp64, in index order, / HW)
int launch_global_avg(const float* x, float* y, long long NC, int HW, hipStream_t s);

// ------------------------------------------------------------------ a net's parameters
struct ConvGeom { int Cin, Cout, kh, kw; };
struct ConvParams { float *wp = nullptr, *alpha = nullptr, *beta = nullptr; int* tab = nullptr; };      // alpha / beta: null where the layer has none

// Writes a net's conv layers into ONE device blob: begin() sizes it (floats_needed per layer plus whatever else the net keeps there) and
// one raw upload buffer for the largest weight; conv() uploads a layer at the cursor, packs it and synchronises (the raw buffer and the
// caller's host vectors are reused by the next layer).  `who` prefixes the error messages.
struct ParamBlob {
    hipStream_t s;
    const char* who;
    float* cursor = nullptr;
    float* raw = nullptr;
    ParamBlob(hipStream_t stream, const char* name) : s(stream), who(name) {}
    ~ParamBlob();
    static size_t floats_needed(const ConvGeom& g);
    int begin(float** params, size_t floats, size_t raw_floats);
    float* take(int n);      // n floats at the cursor, rounded up to 4
    int conv(const ConvGeom& g, const float* w, const float* alpha, const float* beta, ConvParams* out);
};

// ------------------------------------------------------------------ a net's workspaces and tables
// A workspace that only grows (sizes in bytes): nothing happens while *have >= need; else synchronise, free, allocate, *have = need.
int grow(void** ptr, size_t* have, size_t need, hipStream_t s);

// Device tables by input size, built on the host at first sight (build fills `host` and returns one int kept beside the table),
// uploaded, synchronised; freed with the cache.
struct TableCache {
    struct Entry { int* dev; int aux; };
    std::map<int, Entry> map;
    ~TableCache();
    int get(int size, int (*build)(int size, std::vector<int>& host), hipStream_t s, const Entry** out);
};

// One axis of F.interpolate(mode='bilinear', align_corners=False) from S to O positions by torch's coordinate rule:
// src = fl32(scale32 * (d + 0.5) - 0.5) with ONE rounding, scale32 = fl32(S / O); max(src, 0); i0 = floor(src); i1 = min(i0 + 1, S - 1);
// l1 = src - i0 in fp32; l0 = 1 - l1.  Four arrays of O entries.
void bilinear_axis_table(int S, int O, int* i0, int* i1, float* l0, float* l1);

}  // namespace mcvd
