// The FID InceptionV3 (kernels/inception.cpp): the net object behind mcvd_inception_* and its 299 x 299 bilinear resize.  Its convs and
// pools are the detector nets' shared ones (detector_ops.h).
//
// Workspace bound: images are processed in chunks of at most INCEPTION_CHUNK images.  The net always runs at 299 x 299 (resize_input, or
// a 299 x 299 input), so a chunk of n images holds fixed-size maps: the 3 x 299 x 299 input (268 203 floats), two ping-pong maps for the
// trunk (1 382 976 and 967 872: 64 x 147 x 147 and 192 x 71 x 71), two branch temporaries (78 400 and 117 600: 64 and 96 x 35 x 35), the
// pooled branch input (352 800: 288 x 35 x 35) and the outputs of blocks 0-2 (341 056, 235 200, 221 952) -- 3 966 059 floats (15.9 MB)
// per image, 508 MB for a full chunk, whatever n, H and W are.  It is allocated on the first call (for min(n, INCEPTION_CHUNK) images)
// and grows only when a later call brings a larger chunk; the frame size only adds one 4.8 KB coordinate table per distinct H or W,
// built on first sight.  A requested block output is written straight into the caller's buffer.
#pragma once
#include <string>
#include <vector>

#include "detector_ops.h"

struct mcvd_ctx;

namespace mcvd {

constexpr int INCEPTION_SIZE = 299;       // F.interpolate(size=(299, 299)), evaluation/inception.py:147-150
constexpr int INCEPTION_CHUNK = 32;       // images per pass over the net: 17 x 17 maps then give 219 workgroups, 8 x 8 maps 96 and up
constexpr int INCEPTION_BLOCKS = 4;

struct IncLayer { std::string name; int Cin, Cout, kh, kw, stride, ph, pw; };      // one BasicConv2d: conv (no bias) + BN(eps 0.001) + ReLU
struct IncOp { int kind, layer, src, dst, c0, Csrc, Cdst, H, W, block; };         // H, W: the op's input map; c0: first channel of dst written

// One axis of F.interpolate(mode='bilinear', align_corners=False) from S to 299 (bilinear_axis_table, detector_ops.h):
// tab = i0 [299] | i1 [299] | l0 [299] | l1 [299] (the weights as fp32 bit patterns)
void inception_axis_table(int S, std::vector<int>& tab);
// y [n, 3, 299, 299] = (normalize ? 2 v - 1 : v), v = the bilinear resize of x [n, 3, H, W]; tab_h / tab_w: device tables of H and W
int launch_inception_prep(const float* x, float* y, long long n, int H, int W, int normalize, const int* tab_h, const int* tab_w, hipStream_t s);

const std::vector<IncLayer>& inception_layers();

}  // namespace mcvd

struct mcvd_inception {
    mcvd_ctx* ctx = nullptr;
    bool finalized = false;
    std::vector<std::vector<float>> w, bn_w, bn_b, bn_m, bn_v;      // host copies until finalize, one per layer
    float* params = nullptr;                                        // device: packed weights, alpha, beta, tap tables
    std::vector<mcvd::ConvParams> conv;
    float* ws = nullptr;                                            // chunk workspace (see the bound above)
    size_t ws_bytes = 0;
    mcvd::TableCache axis;                                          // input length -> device coordinate table
    mcvd_inception();
    ~mcvd_inception();
};

namespace mcvd {
int inception_set_param(mcvd_inception* n, const char* name, const float* host, int64_t numel);
int inception_finalize(mcvd_inception* n);
int inception_forward(mcvd_inception* n, const float* images01, int64_t count, int H, int W, int resize_input, int normalize_input,
                      int block_mask, float* const* out);
}  // namespace mcvd
