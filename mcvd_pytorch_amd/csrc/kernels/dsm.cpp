// Denoising score-matching loss of NCSNRunner.test() (losses/dsm.py:7-52, versions DDPM / DDIM / FPNDM), forward only, on the device:
//
//   a_b  = alphas[labels[b]]
//   z    = randn_like(x), or under gamma (g - k_cum[t] * theta_t[t]) / sqrt(1 - a_b) with g ~ Gamma(k_cum[t], scale theta_t[t])   :30-36
//   perturbed_x = sqrt(a_b) * x + sqrt(1 - a_b) * z                                                                                :37
//   eps  = scorenet(perturbed_x, labels, cond=cond, cond_mask=cond_mask)          (the model's forward, between the two steps here)
//   loss_b = sum over the row of 1/2 * (z - eps)^2, or |z - eps| under training.L1                                               :41-47
//
// dsm_perturb_kernel: one pass over x, a float4 per lane.  The coefficients are torch's fp32 CPU values: each sqrt correctly rounded
// (evaluated in fp64 and rounded once, which is exact rounding for an fp32 argument), 1 - a rounded to fp32 before it; the gamma
// standardisation divides the same way.  The unit is compiled with -ffp-contract=off (csrc/build.py), so the two products and their
// sum keep the reference's separate roundings.  z is the caller's buffer or Philox keyed by (seed, sample_offset + row, DSM_DRAW,
// element): the GLOBAL row, so a sharded evaluation draws the same z for a row whatever the shard.
// dsm_loss_part_kernel + dsm_loss_final_kernel: the fp32 terms the reference forms (d = z - eps, 0.5f * (d * d) or |d|), summed in fp64
// and rounded once per row.  A row is split over `parts` workgroups so that small batches still fill the device (config 5 evaluates
// B = 8 rows of 245 760 elements); each writes one fp64 partial and the second launch adds a row's partials in index order:
// bit-identical run to run.
#include "../common.h"
#include "philox.h"

namespace mcvd {
namespace {

constexpr uint64_t DSM_DRAW = 1ull << 40;      // draw word of the loss's z (philox.h lists the words in use)
constexpr int DSM_THREADS = 256;
constexpr int DSM_TARGET_BLOCKS = 2048;        // partial-sum workgroups per call: 8 per CU of the 256

__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

struct PerturbArgs {
    const float* x;
    const float* zin;          // NULL: Philox; gamma: the raw draw g
    const int64_t* labels;
    const float* alphas;
    const float* k_cum;        // gamma tables (NULL without gamma)
    const float* theta;
    float* z;
    float* px;
    int T, gamma;
    int64_t per, n4;
    uint64_t seed, sample_offset;
};

__global__ __launch_bounds__(DSM_THREADS) void dsm_perturb_kernel(PerturbArgs a) {
    for (int64_t i = blockIdx.x * (int64_t)DSM_THREADS + threadIdx.x; i < a.n4; i += (int64_t)gridDim.x * DSM_THREADS) {
        const int64_t e = i * 4;
        const int64_t row = e / a.per;                  // per % 4 == 0: the four elements share the row
        int64_t t = a.labels[row];
        t = t < 0 ? t + a.T : t;                        // torch indexing wraps negative labels
        t = t < 0 ? 0 : (t >= a.T ? a.T - 1 : t);
        const float al = a.alphas[t];
        const float sa = sqrt_rn(al), sb = sqrt_rn(1.0f - al);
        const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
        float4 zv;
        if (a.gamma) {
            const float k = a.k_cum[t], th = a.theta[t];
            const float kt = k * th;                    // used_k * used_theta
            const int64_t el = e - row * a.per;
            float g[4];
            if (a.zin) {
                const float4 r = reinterpret_cast<const float4*>(a.zin)[i];
                g[0] = r.x; g[1] = r.y; g[2] = r.z; g[3] = r.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    g[j] = (float)((double)th * philox_gamma64(k, a.seed, a.sample_offset + (uint64_t)row, DSM_DRAW, (uint64_t)(el + j)));
            }
            zv = make_float4(div_rn(g[0] - kt, sb), div_rn(g[1] - kt, sb), div_rn(g[2] - kt, sb), div_rn(g[3] - kt, sb));
        } else if (a.zin) {
            zv = reinterpret_cast<const float4*>(a.zin)[i];
        } else {
            zv = philox_normal4(a.seed, a.sample_offset + (uint64_t)row, DSM_DRAW, (uint64_t)((e - row * a.per) >> 2));
        }
        const float4 pv = make_float4(sa * xv.x + sb * zv.x, sa * xv.y + sb * zv.y, sa * xv.z + sb * zv.z, sa * xv.w + sb * zv.w);
        reinterpret_cast<float4*>(a.z)[i] = zv;
        reinterpret_cast<float4*>(a.px)[i] = pv;
    }
}

__device__ __forceinline__ double dsm_term(float z, float e, int l1) {
    const float d = z - e;
    return (double)(l1 ? fabsf(d) : 0.5f * (d * d));
}

// workgroup (row, p) sums float4s [p * chunk4, min((p + 1) * chunk4, per4)) of its row
__global__ __launch_bounds__(DSM_THREADS) void dsm_loss_part_kernel(const float* __restrict__ z, const float* __restrict__ eps, int64_t per4,
                                                                    int parts, int64_t chunk4, int l1, double* __restrict__ part) {
    __shared__ double red[DSM_THREADS];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / parts;
    const int64_t p = blockIdx.x % parts;
    const int64_t b0 = p * chunk4, b1 = min(per4, b0 + chunk4);
    const float4* zr = reinterpret_cast<const float4*>(z) + row * per4;
    const float4* er = reinterpret_cast<const float4*>(eps) + row * per4;
    double acc = 0.0;
    for (int64_t i = b0 + tid; i < b1; i += DSM_THREADS) {
        const float4 zv = zr[i], ev = er[i];
        acc += dsm_term(zv.x, ev.x, l1) + dsm_term(zv.y, ev.y, l1) + dsm_term(zv.z, ev.z, l1) + dsm_term(zv.w, ev.w, l1);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = DSM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// one workgroup per row: the row's partials are loaded in parallel into LDS, then added by one lane in index order (a serial loop over
// global memory took 20 us at config 5's 240 partials per row, measured)
__global__ __launch_bounds__(DSM_THREADS) void dsm_loss_final_kernel(const double* __restrict__ part, int parts, float* __restrict__ out) {
    __shared__ double p[DSM_TARGET_BLOCKS];
    const int64_t row = blockIdx.x;
    for (int k = threadIdx.x; k < parts; k += DSM_THREADS) p[k] = part[row * parts + k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < parts; ++k) s += p[k];
        out[row] = (float)s;
    }
}

}  // namespace

int dsm_loss_parts(int B, int64_t per) {
    const int64_t per4 = per / 4;
    int64_t p = (DSM_TARGET_BLOCKS + B - 1) / B;
    const int64_t cap = (per4 + DSM_THREADS - 1) / DSM_THREADS;     // at least one float4 per lane
    if (p > cap) p = cap;
    return (int)(p < 1 ? 1 : p);
}

int launch_dsm_perturb(const float* x, const float* zin, const int64_t* labels, const float* alphas, const float* k_cum, const float* theta,
                       int T, int gamma, uint64_t seed, uint64_t sample_offset, int B, int64_t per, float* z, float* px, hipStream_t s) {
    MCVD_REQUIRE(x && labels && alphas && z && px && B > 0 && per > 0 && T > 0, "dsm_perturb: bad arguments");
    MCVD_REQUIRE(per % 4 == 0, "dsm_perturb: %lld elements per row is not a multiple of 4", (long long)per);
    MCVD_REQUIRE(!gamma || (k_cum && theta), "dsm_perturb: gamma needs the k_cum / theta_t tables");
    PerturbArgs a{x, zin, labels, alphas, k_cum, theta, z, px, T, gamma, per, (int64_t)B * per / 4, seed, sample_offset};
    const int64_t blocks = (a.n4 + DSM_THREADS - 1) / DSM_THREADS;
    hipLaunchKernelGGL(dsm_perturb_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(DSM_THREADS), 0, s, a);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_dsm_loss(const float* z, const float* eps, int B, int64_t per, int l1, double* part, float* loss_rows, hipStream_t s) {
    MCVD_REQUIRE(z && eps && part && loss_rows && B > 0 && per > 0 && per % 4 == 0, "dsm_loss: bad arguments");
    const int parts = dsm_loss_parts(B, per);
    const int64_t per4 = per / 4, chunk4 = (per4 + parts - 1) / parts;
    const int64_t blocks = (int64_t)B * parts;
    MCVD_REQUIRE(blocks < (1LL << 31), "dsm_loss: %lld workgroups exceed one launch", (long long)blocks);
    hipLaunchKernelGGL(dsm_loss_part_kernel, dim3((unsigned)blocks), dim3(DSM_THREADS), 0, s, z, eps, per4, parts, chunk4, l1, part);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dsm_loss_final_kernel, dim3((unsigned)B), dim3(DSM_THREADS), 0, s, part, parts, loss_rows);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mcvd
