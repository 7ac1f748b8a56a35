// LPIPS v0.1 on the AlexNet feature stack (kernels/lpips.cpp): the net object behind mcvd_lpips_*.  Its convs and pools are the detector
// nets' shared ones (detector_ops.h).
//
// Workspace bound: frames are processed in chunks of at most LPIPS_CHUNK frames.  A chunk of n frames holds, for its 2 n images, the
// normalised 3 x 128 x 128 input and the five taps with the two pooled maps between them: 443 136 floats (1.77 MB) per frame, plus
// 5 floats per frame of per-tap values and 2 * C * H * 128 bytes per frame of uint8 rows between the two resize passes -- at most
// 114 MB + 64 * 256 * C * H bytes, whatever B * T is.  It is allocated on the first call (for min(B * T, LPIPS_CHUNK) frames) and grows
// only when a later call brings a larger chunk or taller frames; the resize tables are built once per input size.
#pragma once
#include <string>
#include <vector>

#include "detector_ops.h"

struct mcvd_ctx;

namespace mcvd {

constexpr int LPIPS_SIZE = 128;       // Resize((128, 128)), runners/ncsn_runner.py:1427
constexpr int LPIPS_CHUNK = 64;       // frames per pass over the net
constexpr int LPIPS_TAPS = 5;

struct LpipsLayer { int feat, slice, Cin, Cout, ks, stride, pad, H, OH, pool; };      // pool: MaxPool2d(3, 2) in front (H is the conv's input size)
extern const LpipsLayer LPIPS_LAYERS[LPIPS_TAPS];

}  // namespace mcvd

struct mcvd_lpips {
    mcvd_ctx* ctx = nullptr;
    bool finalized = false;
    std::vector<float> w[mcvd::LPIPS_TAPS], b[mcvd::LPIPS_TAPS], lin[mcvd::LPIPS_TAPS], shift, scale;      // host copies until finalize
    float* params = nullptr;                                     // device: packed weights, biases (the convs' beta), tap tables, lin vectors
    mcvd::ConvParams conv[mcvd::LPIPS_TAPS];
    float* lind[mcvd::LPIPS_TAPS] = {};
    float sh[3] = {}, sc[3] = {};
    float* ws = nullptr;                                         // chunk workspace (see the bound above)
    size_t ws_bytes = 0;
    unsigned char* rows = nullptr;                               // uint8 result of the horizontal resize pass
    size_t rows_bytes = 0;
    mcvd::TableCache tabs;                                       // input size -> (device table: first tap | tap count | coefficients, taps per output)
    ~mcvd_lpips();
};

namespace mcvd {
int lpips_set_param(mcvd_lpips* n, const char* name, const float* host, int64_t numel);
int lpips_finalize(mcvd_lpips* n);
int lpips_frames(mcvd_lpips* n, const float* pred01, const float* real01, int B, int T, int C, int H, int W, float* lpips_out,
                 unsigned char* resized_out, float* per_tap_out);
}  // namespace mcvd
