// Per-frame MSE and SSIM of video_gen's test mode (runners/ncsn_runner.py:1580-1609, :1749-1778), on the device.
//
// For frame jj of row ii the reference takes the C channels jj*C .. jj*C+C-1 of pred / real ([B, T*C, H, W] in [0, 1]) and computes
//   mse  = F.mse_loss(real_ij, pred_ij)                                 fp32 difference; here squared and summed in fp64, rounded once
//   grey = ToPILImage()(x).convert("RGB").convert("L")                  x.mul(255).byte() (one fp32 multiply, truncation), then Pillow's
//                                                                       luma (19595 R + 38470 G + 7471 B + 0x8000) >> 16; C = 1 is its own grey
//          (MNIST datasets: torch.round(x) first -- round half to even, rintf)
//   ssim = skimage structural_similarity(grey_p, grey_r, data_range=255, gaussian_weights=True, use_sample_covariance=False):
//          Gaussian moments (sigma 1.5, truncate 3.5: 11 taps) of X, Y, X^2, Y^2, XY in fp64, S per pixel, mean over the interior
//          with a 5-pixel border cropped.  The interior reads no pixel outside the frame, so no border mode is involved.
//
// Two launches: frame_ssim_tile_kernel writes one fp64 partial sum of S per (frame, tile); frame_finalize_kernel (one workgroup per frame)
// reduces the frame's MSE and adds the tile partials in index order.  Every sum has a fixed order: results are bit-identical run to run.
#include "../common.h"

namespace mcvd {
namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_TW = 64;                  // interior columns per tile
constexpr int MT_SR = 12;                  // interior rows per tile
constexpr int MT_R = 5;                    // window radius (win_size 11)
constexpr int MT_IR = MT_SR + 2 * MT_R;    // grey rows a tile reads
constexpr int MT_IC = MT_TW + 2 * MT_R;    // grey columns a tile reads

struct GaussTaps { double w[MT_R + 1]; };  // w[k] = weight of offset +-k (symmetric window)

// x.mul(255).byte(), with torch.round(x) first under the MNIST rule.  Inputs are in [0, 1]; the clamp only defines what lies outside.
__device__ __forceinline__ int quantise(float x, bool binary) {
    if (binary) x = rintf(x);
    const float v = __fmul_rn(x, 255.0f);
    return (int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// grey level of pixel p of a frame whose C planes start at f (plane stride HW)
__device__ __forceinline__ int grey_at(const float* f, int64_t p, int64_t HW, int C, bool binary) {
    if (C == 1) return quantise(f[p], binary);
    const int r = quantise(f[p], binary), g = quantise(f[p + HW], binary), b = quantise(f[p + 2 * HW], binary);
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
}

__global__ __launch_bounds__(MT_THREADS) void frame_ssim_tile_kernel(const float* __restrict__ pred, const float* __restrict__ real, int C,
                                                                       int H, int W, int ntx, int ntiles, int binary, GaussTaps taps,
                                                                       double* __restrict__ part) {
    __shared__ unsigned char gp[MT_IR][MT_IC], gr[MT_IR][MT_IC];
    __shared__ double hm[5][MT_IR][MT_TW];            // row-filtered moments: X, Y, X^2, Y^2, XY
    __shared__ double red[MT_THREADS];
    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int tx = tile % ntx, ty = tile / ntx;
    const int x0 = tx * MT_TW, y0 = ty * MT_SR;       // first grey column / row the tile reads (= its first interior pixel - 5)
    const int ow = min(MT_TW, W - 2 * MT_R - x0), oh = min(MT_SR, H - 2 * MT_R - y0);
    const int iw = ow + 2 * MT_R, ih = oh + 2 * MT_R;
    const int64_t HW = (int64_t)H * W;
    const float* fp = pred + frame * C * HW;
    const float* fr = real + frame * C * HW;
    const bool bin = binary != 0;

    for (int i = tid; i < ih * iw; i += MT_THREADS) {
        const int r = i / iw, c = i % iw;
        const int64_t p = (int64_t)(y0 + r) * W + x0 + c;
        gp[r][c] = (unsigned char)grey_at(fp, p, HW, C, bin);
        gr[r][c] = (unsigned char)grey_at(fr, p, HW, C, bin);
    }
    __syncthreads();

    for (int i = tid; i < ih * ow; i += MT_THREADS) {
        const int r = i / ow, c = i % ow + MT_R;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
        for (int k = -MT_R; k <= MT_R; ++k) {
            const double w = taps.w[k < 0 ? -k : k];
            const double x = (double)gp[r][c + k], y = (double)gr[r][c + k];
            sx = fma(w, x, sx);
            sy = fma(w, y, sy);
            sxx = fma(w, x * x, sxx);
            syy = fma(w, y * y, syy);
            sxy = fma(w, x * y, sxy);
        }
        const int cc = c - MT_R;
        hm[0][r][cc] = sx; hm[1][r][cc] = sy; hm[2][r][cc] = sxx; hm[3][r][cc] = syy; hm[4][r][cc] = sxy;
    }
    __syncthreads();

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double acc = 0.0;
    for (int i = tid; i < oh * ow; i += MT_THREADS) {
        const int r = i / ow + MT_R, c = i % ow;
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
        for (int k = -MT_R; k <= MT_R; ++k) {
            const double w = taps.w[k < 0 ? -k : k];
            ux = fma(w, hm[0][r + k][c], ux);
            uy = fma(w, hm[1][r + k][c], uy);
            uxx = fma(w, hm[2][r + k][c], uxx);
            uyy = fma(w, hm[3][r + k][c], uyy);
            uxy = fma(w, hm[4][r + k][c], uxy);
        }
        // skimage: vx = cov_norm * (uxx - ux * ux), cov_norm = 1 (use_sample_covariance=False)
        const double vx = uxx - ux * ux, vy = uyy - uy * uy, vxy = uxy - ux * uy;
        const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2;
        const double b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
        acc += (a1 * a2) / (b1 * b2);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) part[frame * ntiles + tile] = red[0];
}

__global__ __launch_bounds__(MT_THREADS) void frame_finalize_kernel(const float* __restrict__ pred, const float* __restrict__ real, int64_t n,
                                                                      const double* __restrict__ part, int ntiles, double n_interior,
                                                                      float* __restrict__ mse_out, double* __restrict__ ssim_out) {
    __shared__ double red[MT_THREADS];
    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.x;
    const float* fp = pred + frame * n;
    const float* fr = real + frame * n;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += MT_THREADS) {
        const double d = (double)__fsub_rn(fr[i], fp[i]);          // F.mse_loss(real_ij, pred_ij): real - pred, rounded to fp32
        acc = fma(d, d, acc);                                        // d * d is exact in fp64
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < ntiles; ++k) s += part[frame * ntiles + k];
        mse_out[frame] = (float)(red[0] / (double)n);
        ssim_out[frame] = s / n_interior;
    }
}

// grey_out: [2, frames, H, W] uint8 -- the planes of pred, then of real (test aid)
__global__ __launch_bounds__(MT_THREADS) void frame_grey_kernel(const float* __restrict__ pred, const float* __restrict__ real, int C, int64_t HW,
                                                                  int64_t npix, int binary, unsigned char* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)MT_THREADS + threadIdx.x; i < npix; i += (int64_t)gridDim.x * MT_THREADS) {
        const int64_t frame = i / HW, p = i % HW;
        out[i] = (unsigned char)grey_at(pred + frame * C * HW, p, HW, C, binary != 0);
        out[npix + i] = (unsigned char)grey_at(real + frame * C * HW, p, HW, C, binary != 0);
    }
}

}  // namespace

int64_t frame_metrics_scratch_bytes(int frames, int H, int W) {
    const int64_t ntx = (W - 2 * MT_R + MT_TW - 1) / MT_TW, nty = (H - 2 * MT_R + MT_SR - 1) / MT_SR;
    return (int64_t)frames * ntx * nty * (int64_t)sizeof(double);
}

int launch_frame_metrics(const float* pred, const float* real, int frames, int C, int H, int W, int binary, float* mse_out, double* ssim_out,
                         unsigned char* grey_out, double* part, hipStream_t s) {
    MCVD_REQUIRE(pred && real && mse_out && ssim_out && part, "frame_metrics: NULL argument");
    MCVD_REQUIRE(frames > 0 && (C == 1 || C == 3) && H >= 2 * MT_R + 1 && W >= 2 * MT_R + 1, "frame_metrics: bad shape");
    const int ntx = (W - 2 * MT_R + MT_TW - 1) / MT_TW, nty = (H - 2 * MT_R + MT_SR - 1) / MT_SR;
    const int64_t blocks = (int64_t)frames * ntx * nty;
    MCVD_REQUIRE(blocks < (1LL << 31), "frame_metrics: %lld tiles exceed one launch", (long long)blocks);
    // scipy.ndimage._gaussian_kernel1d(1.5, 0, 5): exp(-0.5 / sigma^2 * x^2) over x = -5..5, normalised
    GaussTaps taps;
    double e[MT_R + 1], sum = 0.0;
    for (int k = 0; k <= MT_R; ++k) e[k] = exp(-0.5 / (1.5 * 1.5) * (double)(k * k));
    for (int x = -MT_R; x <= MT_R; ++x) sum += e[x < 0 ? -x : x];
    for (int k = 0; k <= MT_R; ++k) taps.w[k] = e[k] / sum;
    hipLaunchKernelGGL(frame_ssim_tile_kernel, dim3((unsigned)blocks), dim3(MT_THREADS), 0, s, pred, real, C, H, W, ntx, ntx * nty, binary, taps,
                       part);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(frame_finalize_kernel, dim3((unsigned)frames), dim3(MT_THREADS), 0, s, pred, real, (int64_t)C * H * W, part, ntx * nty,
                       (double)(H - 2 * MT_R) * (double)(W - 2 * MT_R), mse_out, ssim_out);
    MCVD_HIP_CHECK(hipGetLastError());
    if (grey_out) {
        const int64_t npix = (int64_t)frames * H * W;
        const int grid = (int)((npix + MT_THREADS - 1) / MT_THREADS > 16384 ? 16384 : (npix + MT_THREADS - 1) / MT_THREADS);
        hipLaunchKernelGGL(frame_grey_kernel, dim3(grid), dim3(MT_THREADS), 0, s, pred, real, C, (int64_t)H * W, npix, binary, grey_out);
        MCVD_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace mcvd
