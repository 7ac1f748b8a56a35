// The two device steps of video_gen's FVD path that surround the detector call (the detector itself comes from the caller).
//
// fvd_clips_kernel: the detector's input in one pass -- the torch.cat of cond | pred-or-real | future frames, the [::preds_per_test] row
//   selection, to_i3d (grey repeated to RGB, BTCHW -> BCTHW; runners/ncsn_runner.py:1918-1982) and preprocess_single (models/fvd/fvd.py:160-186)
//   for square frames: F.interpolate(mode='bilinear', align_corners=False) to 224 x 224 (the centre crop is then the identity) and
//   (v - 0.5) * 2.  Per-axis tables (two source indices and two fp32 weights per output position) come from the host with torch's
//   coordinate rule (bilinear_axis_table, detector_ops.h).  The lerp has torch's order, every operation rounded separately:
//   h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11).  One thread per four consecutive output pixels (224 = 56 * 4), float4 stores;
//   a grey value is computed once and stored to the three channel planes.
//
// feature_stats: np.mean(axis=0) and np.cov(rowvar=False) (fvd.py:275-278) of the rows row_start, row_start + row_step, ... of a feature
//   matrix, all sums in fp64, two passes as np.cov makes them.  Rows are split into G chunks, G a function of (rows, d) only; every chunk
//   sum has a fixed order and the chunk partials are added in index order: bit-identical run to run.  The centred product runs on
//   v_mfma_f64_16x16x4_f64, one wave per (16 x 16 tile of the lower triangle, chunk); the upper triangle is the mirror of the lower, so
//   sigma is exactly symmetric.
#include "../detector_ops.h"

namespace mcvd {
namespace {

constexpr int FV_OUT = 224;                 // preprocess_single's resolution
constexpr int FV_Q = FV_OUT / 4;            // float4 groups per output row
constexpr int FV_THREADS = 256;

struct FvdTable {                           // per output position of one axis (frames are square: rows and columns share it)
    unsigned short i0[FV_OUT], i1[FV_OUT];
    float l0[FV_OUT], l1[FV_OUT];
};

struct FvdParts {
    const float* ptr[3];
    int64_t bstride[3];                     // floats between two rows of the batch
    int first[3];                           // first output frame of the part
    int nparts;
};

__device__ __forceinline__ float lerp_px(const float* __restrict__ r0, const float* __restrict__ r1, int x0, int x1, float w0, float w1, float h0,
                                          float h1) {
    const float top = __fadd_rn(__fmul_rn(w0, r0[x0]), __fmul_rn(w1, r0[x1]));
    const float bot = __fadd_rn(__fmul_rn(w0, r1[x0]), __fmul_rn(w1, r1[x1]));
    const float v = __fadd_rn(__fmul_rn(h0, top), __fmul_rn(h1, bot));
    return __fmul_rn(__fsub_rn(v, 0.5f), 2.0f);
}

// out: [Bsel, 3, T, 224, 224].  planes = 3 for C = 3 (one thread group per channel plane), 1 for C = 1 (computed once, stored three times)
__global__ __launch_bounds__(FV_THREADS) void fvd_clips_kernel(FvdParts parts, FvdTable tab, int C, int S, int T, int row_start, int row_step,
                                                                 int64_t total, float* __restrict__ out) {
    __shared__ FvdTable t;
    for (int i = threadIdx.x; i < FV_OUT; i += FV_THREADS) {
        t.i0[i] = tab.i0[i];
        t.i1[i] = tab.i1[i];
        t.l0[i] = tab.l0[i];
        t.l1[i] = tab.l1[i];
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * FV_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)(idx % FV_Q);
    const int y = (int)((idx / FV_Q) % FV_OUT);
    int64_t rest = idx / (FV_Q * FV_OUT);
    const int tt = (int)(rest % T);
    rest /= T;
    const int planes = C == 3 ? 3 : 1;
    const int c = (int)(rest % planes);
    const int64_t b = rest / planes;

    int k = 0;
    if (parts.nparts > 1 && tt >= parts.first[1]) k = 1;
    if (parts.nparts > 2 && tt >= parts.first[2]) k = 2;
    const int64_t SS = (int64_t)S * S;
    const float* src = parts.ptr[k] + (row_start + b * row_step) * parts.bstride[k] + ((int64_t)(tt - parts.first[k]) * C + c) * SS;
    const float* r0 = src + (int64_t)t.i0[y] * S;
    const float* r1 = src + (int64_t)t.i1[y] * S;
    const float h0 = t.l0[y], h1 = t.l1[y];
    float4 v;
    const int x = 4 * q;
    v.x = lerp_px(r0, r1, t.i0[x], t.i1[x], t.l0[x], t.l1[x], h0, h1);
    v.y = lerp_px(r0, r1, t.i0[x + 1], t.i1[x + 1], t.l0[x + 1], t.l1[x + 1], h0, h1);
    v.z = lerp_px(r0, r1, t.i0[x + 2], t.i1[x + 2], t.l0[x + 2], t.l1[x + 2], h0, h1);
    v.w = lerp_px(r0, r1, t.i0[x + 3], t.i1[x + 3], t.l0[x + 3], t.l1[x + 3], h0, h1);
    const int64_t plane = (int64_t)FV_OUT * FV_OUT;
    const int64_t o = ((b * 3 + c) * T + tt) * plane + (int64_t)y * FV_OUT + x;
    *reinterpret_cast<float4*>(out + o) = v;
    if (C == 1) {
        *reinterpret_cast<float4*>(out + o + (int64_t)T * plane) = v;
        *reinterpret_cast<float4*>(out + o + 2 * (int64_t)T * plane) = v;
    }
}

// ---- feature statistics ---------------------------------------------------------------------------------------------------------------

constexpr int FS_THREADS = 256;

template <typename T>
__device__ __forceinline__ double fs_load(const void* x, int64_t i) { return (double)static_cast<const T*>(x)[i]; }

// part[g * d + c] = sum of column c over the selected rows of chunk g, in row order
template <typename T>
__global__ __launch_bounds__(FS_THREADS) void fs_colsum_kernel(const void* __restrict__ x, int64_t ld, int64_t row_start, int64_t row_step, int n,
                                                                 int d, int chunk, double* __restrict__ part) {
    const int c = blockIdx.x * FS_THREADS + threadIdx.x;
    const int g = blockIdx.y;
    if (c >= d) return;
    const int r1 = min(n, (g + 1) * chunk);
    double s = 0.0;
    for (int r = g * chunk; r < r1; ++r) s += fs_load<T>(x, (row_start + (int64_t)r * row_step) * ld + c);
    part[(int64_t)g * d + c] = s;
}

__global__ __launch_bounds__(FS_THREADS) void fs_mean_kernel(const double* __restrict__ part, int G, int n, int d, double* __restrict__ mean) {
    const int c = blockIdx.x * FS_THREADS + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(int64_t)g * d + c];
    mean[c] = s / (double)n;
}

// One wave per (lower-triangle tile, chunk): acc[ti*16 + i][tj*16 + j] = sum over the chunk's rows of xc[r][i] * xc[r][j], four rows per
// MFMA.  v_mfma_f64_16x16x4_f64: lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result register v of lane l is
// C[row (l >> 4) + 4 v][col l & 15].  Columns at or beyond d and rows beyond the chunk enter as zeros.
template <typename T>
__global__ __launch_bounds__(64) void fs_cov_tile_kernel(const void* __restrict__ x, int64_t ld, int64_t row_start, int64_t row_step, int n, int d,
                                                          int chunk, const double* __restrict__ mean, double* __restrict__ part) {
    const int tile = blockIdx.x, g = blockIdx.y;
    // tile -> (ti >= tj) of the lower triangle: tile = ti * (ti + 1) / 2 + tj
    int ti = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    while (ti * (ti + 1) / 2 > tile) --ti;
    const int tj = tile - ti * (ti + 1) / 2;
    const int lane = threadIdx.x, lc = lane & 15, lk = lane >> 4;
    const int ca = ti * 16 + lc, cb = tj * 16 + lc;
    const bool va = ca < d, vb = cb < d;
    const double ma = va ? mean[ca] : 0.0, mb = vb ? mean[cb] : 0.0;
    typedef double double4_t __attribute__((ext_vector_type(4)));
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    const int r1 = min(n, (g + 1) * chunk);
    for (int r0 = g * chunk; r0 < r1; r0 += 4) {
        const int r = r0 + lk;
        double a = 0.0, b = 0.0;
        if (r < r1) {
            const int64_t base = (row_start + (int64_t)r * row_step) * ld;
            if (va) a = fs_load<T>(x, base + ca) - ma;
            if (vb) b = fs_load<T>(x, base + cb) - mb;
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double* p = part + ((int64_t)g * gridDim.x + tile) * 256;
    for (int v = 0; v < 4; ++v) p[(lk + 4 * v) * 16 + lc] = acc[v];
}

// sigma[i][j] = sigma[j][i] = (sum over chunks, in index order) * (1 / (n - 1)) for i >= j
__global__ __launch_bounds__(FS_THREADS) void fs_cov_final_kernel(const double* __restrict__ part, int G, int ntiles, int n, int d,
                                                                    double* __restrict__ sigma) {
    const int tile = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    while (ti * (ti + 1) / 2 > tile) --ti;
    const int tj = tile - ti * (ti + 1) / 2;
    const int e = threadIdx.x, i = ti * 16 + e / 16, j = tj * 16 + e % 16;
    if (i >= d || j >= d || j > i) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[((int64_t)g * ntiles + tile) * 256 + e];
    const double v = s * (1.0 / (double)(n - 1));                 // np.cov: c *= np.true_divide(1, fact)
    sigma[(int64_t)i * d + j] = v;
    sigma[(int64_t)j * d + i] = v;
}

int fs_tiles(int d) {
    const int t = (d + 15) / 16;
    return t * (t + 1) / 2;
}

// chunks of the covariance pass: about 128 rows each, at most 2048 waves in all (one chunk where the triangle alone has more tiles)
int fs_chunks(int n, int d) {
    const int cap = 2048 / fs_tiles(d) > 1 ? 2048 / fs_tiles(d) : 1;
    const int want = (n + 127) / 128;
    return want < cap ? want : cap;
}

}  // namespace

int launch_fvd_clips(const float* const* parts, const int* frames, const int64_t* bstride, int nparts, int Bsel, int row_start, int row_step,
                     int C, int S, float* out, hipStream_t s) {
    MCVD_REQUIRE(parts && frames && bstride && out, "fvd_clips: NULL argument");
    MCVD_REQUIRE(nparts >= 1 && nparts <= 3, "fvd_clips: %d parts (1 to 3: cond, pred or real, future)", nparts);
    MCVD_REQUIRE(C == 1 || C == 3, "fvd_clips: channels must be 1 or 3, got %d", C);
    MCVD_REQUIRE(S >= 1 && S <= 32768, "fvd_clips: bad frame size %d", S);
    MCVD_REQUIRE(Bsel > 0 && row_start >= 0 && row_step >= 1, "fvd_clips: bad row selection (%d rows from %d, step %d)", Bsel, row_start, row_step);
    FvdParts p;
    int T = 0;
    for (int k = 0; k < 3; ++k) {
        p.ptr[k] = nullptr;
        p.bstride[k] = 0;
        p.first[k] = 0;
    }
    for (int k = 0; k < nparts; ++k) {
        MCVD_REQUIRE(parts[k] && frames[k] > 0, "fvd_clips: part %d is NULL or has %d frames", k, frames[k]);
        MCVD_REQUIRE(bstride[k] >= (int64_t)frames[k] * C * S * S, "fvd_clips: part %d: batch stride %lld is smaller than its frames", k,
                     (long long)bstride[k]);
        p.ptr[k] = parts[k];
        p.bstride[k] = bstride[k];
        p.first[k] = T;
        T += frames[k];
    }
    p.nparts = nparts;
    FvdTable tab;
    int i0[FV_OUT], i1[FV_OUT];
    bilinear_axis_table(S, FV_OUT, i0, i1, tab.l0, tab.l1);
    for (int d = 0; d < FV_OUT; ++d) {      // S <= 32768: the indices fit 16 bits
        tab.i0[d] = (unsigned short)i0[d];
        tab.i1[d] = (unsigned short)i1[d];
    }
    const int64_t total = (int64_t)Bsel * (C == 3 ? 3 : 1) * T * FV_OUT * FV_Q;
    const int64_t blocks = (total + FV_THREADS - 1) / FV_THREADS;
    MCVD_REQUIRE(blocks < (1LL << 31), "fvd_clips: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL(fvd_clips_kernel, dim3((unsigned)blocks), dim3(FV_THREADS), 0, s, p, tab, C, S, T, row_start, row_step, total, out);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t feature_stats_scratch_bytes(int n, int d) {
    const int64_t G1 = (n + 255) / 256;
    const int64_t cov = (int64_t)fs_chunks(n, d) * fs_tiles(d) * 256;
    return (G1 * d > cov ? G1 * d : cov) * (int64_t)sizeof(double);
}

// x: [.., ld] fp32 (is_f64 0) or fp64 (1); n selected rows row_start + r * row_step; mean: [d], sigma: [d, d] fp64
int launch_feature_stats(const void* x, int is_f64, int64_t ld, int64_t row_start, int64_t row_step, int n, int d, double* mean, double* sigma,
                         double* scratch, hipStream_t s) {
    MCVD_REQUIRE(x && mean && sigma && scratch, "feature_stats: NULL argument");
    MCVD_REQUIRE(d >= 1 && d <= 2048 && ld >= d, "feature_stats: bad d = %d (1 to 2048) or leading dimension %lld", d, (long long)ld);
    MCVD_REQUIRE(n >= 2, "feature_stats: %d selected rows (np.cov of fewer than two rows is NaN)", n);
    MCVD_REQUIRE(row_start >= 0 && row_step >= 1, "feature_stats: bad row selection");
    const int G1 = (n + 255) / 256, chunk1 = 256;
    const int G = fs_chunks(n, d), ntiles = fs_tiles(d);
    const int chunk = (((n + G - 1) / G) + 3) / 4 * 4;            // rows per chunk, a multiple of the MFMA's four
    const int cb = (d + FS_THREADS - 1) / FS_THREADS;
    MCVD_REQUIRE(G1 <= 65535, "feature_stats: %d rows exceed one launch", n);
    double* part = scratch;                                        // the column partials, then (the mean written) the tile partials
    if (is_f64)
        hipLaunchKernelGGL(fs_colsum_kernel<double>, dim3(cb, G1), dim3(FS_THREADS), 0, s, x, ld, row_start, row_step, n, d, chunk1, part);
    else
        hipLaunchKernelGGL(fs_colsum_kernel<float>, dim3(cb, G1), dim3(FS_THREADS), 0, s, x, ld, row_start, row_step, n, d, chunk1, part);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fs_mean_kernel, dim3(cb), dim3(FS_THREADS), 0, s, part, G1, n, d, mean);
    MCVD_HIP_CHECK(hipGetLastError());
    if (is_f64)
        hipLaunchKernelGGL(fs_cov_tile_kernel<double>, dim3(ntiles, G), dim3(64), 0, s, x, ld, row_start, row_step, n, d, chunk, mean, part);
    else
        hipLaunchKernelGGL(fs_cov_tile_kernel<float>, dim3(ntiles, G), dim3(64), 0, s, x, ld, row_start, row_step, n, d, chunk, mean, part);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(fs_cov_final_kernel, dim3(ntiles), dim3(FS_THREADS), 0, s, part, G, ntiles, n, d, sigma);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mcvd
