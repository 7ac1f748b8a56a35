// Sampler elementwise kernels: label fill, the fused DDPM/DDIM update (models/__init__.py:287-290, :165-168,
// :324-328), the t_min re-noise (:279), the final denoise (:333), and a counter-based Philox4x32-10 + Box-Muller
// normal generator keyed by (seed, GLOBAL sample index, draw, element) so the stream does not depend on how the
// batch is sharded over GPUs.  The arithmetic keeps the reference's operation order with one rounding per multiply / add
// (CPU torch does not contract to FMA): this translation unit is compiled with -ffp-contract=off (csrc/build.py) -- the
// __fmul_rn / __fadd_rn device functions alone do not prevent contraction, they are inlined under the unit's default.
#include "../common.h"
#include "philox.h"

namespace mcvd {

__global__ __launch_bounds__(256) void gamma_noise_kernel(float* out, const float* raw, float k, float theta, float kt, float sd,
                                                           uint64_t seed, uint64_t sample_offset, uint64_t draw, int64_t n,
                                                           int64_t per_sample) {
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float g;
        if (raw) {
            g = raw[i];
        } else {
            const int64_t row = i / per_sample;
            g = (float)((double)theta * philox_gamma64(k, seed, sample_offset + (uint64_t)row, draw, (uint64_t)(i - row * per_sample)));
        }
        out[i] = (g - kt) / sd;                       // (z - ks_cum[i] * thetas[i]) / (1 - alphas[i]).sqrt()
    }
}

int launch_gamma_noise(float* out, const float* raw, float k, float theta, float kt, float sd, uint64_t seed,
                       uint64_t sample_offset, uint64_t draw, int B, int64_t per_sample, hipStream_t s) {
    MCVD_REQUIRE(out && (raw || (k > 0.0f && theta > 0.0f)) && sd > 0.0f, "gamma_noise: bad arguments (k=%g theta=%g sd=%g)", k, theta, sd);
    const int64_t n = (int64_t)B * per_sample;
    const int grid = (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
    hipLaunchKernelGGL(gamma_noise_kernel, dim3(grid), dim3(256), 0, s, out, raw, k, theta, kt, sd, seed, sample_offset, draw, n,
                       per_sample);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// out[b] = sqrt(a_b) * cond[b] + sqrt(1 - a_b) * z[b],  a_b = alphas[labels[b]]        ncsnpp_more.py:758, :768
__global__ __launch_bounds__(256) void cond_noise_kernel(const float* cond, const float* z, const float* alphas, const int64_t* labels,
                                                          int T, float* out, int64_t n, int64_t per_sample) {
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / per_sample;
        int64_t t = labels[row];
        t = t < 0 ? t + T : t;                        // torch indexing wraps negative labels
        t = t < 0 ? 0 : (t >= T ? T - 1 : t);
        const float a = alphas[t];
        out[i] = sqrtf(a) * cond[i] + sqrtf(1.0f - a) * z[i];
    }
}

int launch_cond_noise(const float* cond, const float* z, const float* alphas_dev, const int64_t* labels, int T, float* out, int B,
                      int64_t per_sample, hipStream_t s) {
    MCVD_REQUIRE(cond && z && alphas_dev && labels && out, "cond_noise: NULL argument");
    const int64_t n = (int64_t)B * per_sample;
    const int grid = (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
    hipLaunchKernelGGL(cond_noise_kernel, dim3(grid), dim3(256), 0, s, cond, z, alphas_dev, labels, T, out, n, per_sample);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// [B, T*C, H, W] float in [0, 1] (after inverse_data_transform) -> [B, T, H, W, C] uint8, `(frame * 255).astype('uint8')`
// (runners/ncsn_runner.py:2019-2062: BCHW -> permute(0, 2, 3, 1) -> * 255 -> astype uint8, truncation toward zero)
__global__ __launch_bounds__(256) void pack_frames_u8_kernel(const float* in, uint8_t* out, int T, int C, int HW, int64_t n) {
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t r = i / C;
        const int p = (int)(r % HW);
        const int64_t bt = r / HW;                        // b * T + t
        const float v = in[(bt * C + c) * HW + p] * 255.0f;
        out[i] = (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
    }
}
int launch_pack_frames_u8(const float* in, uint8_t* out, int B, int T, int C, int HW, hipStream_t s) {
    MCVD_REQUIRE(in && out && B > 0 && T > 0 && C > 0 && HW > 0, "pack_frames_u8: bad arguments");
    const int64_t n = (int64_t)B * T * C * HW;
    const int grid = (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_frames_u8_kernel, dim3(grid), dim3(256), 0, s, in, out, T, C, HW, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void fill_labels_kernel(int64_t* labels, int64_t v, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) labels[i] = v;
}
int launch_fill_labels(int64_t* labels, int64_t value, int B, hipStream_t s) {
    hipLaunchKernelGGL(fill_labels_kernel, dim3((B + 255) / 256), dim3(256), 0, s, labels, value, B);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void fill_labels_f_kernel(float* labels, float v, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) labels[i] = v;
}
int launch_fill_labels_f(float* labels, float value, int B, hipStream_t s) {
    hipLaunchKernelGGL(fill_labels_f_kernel, dim3((B + 255) / 256), dim3(256), 0, s, labels, value, B);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

struct UpdArgs {
    int kind; float* x; const float* eps; const float* noise; float c_x0a, c_x0b, c_mean0, c_mean1, c_noise; int clip;
    int64_t n; int use_philox; uint64_t seed, sample_offset, draw; int64_t per_sample;
};

__global__ __launch_bounds__(256) void sampler_update_kernel(UpdArgs a) {
    const int64_t n4 = a.n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
        const float4 ev = reinterpret_cast<const float4*>(a.eps)[i];
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.c_noise != 0.0f) {
            if (a.use_philox) {
                const int64_t e = i * 4;
                const int64_t row = e / a.per_sample;
                zv = philox_normal4(a.seed, a.sample_offset + (uint64_t)row, a.draw, (uint64_t)((e - row * a.per_sample) >> 2));
            } else {
                zv = reinterpret_cast<const float4*>(a.noise)[i];
            }
        }
        float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w}, zs[4] = {zv.x, zv.y, zv.z, zv.w}, o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // x0 = (1/sqrt(a)) * (x - sqrt(1-a)*eps)                                   :287 / :165
            float x0 = __fmul_rn(a.c_x0a, __fsub_rn(xs[j], __fmul_rn(a.c_x0b, es[j])));
            if (a.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);                              // :288-289
            // ddpm: c_mean0*x0 + c_mean1*x (:290)      ddim: c_mean0*x0 + c_mean1*eps (:168)
            const float second = (a.kind == 0) ? xs[j] : es[j];
            float v = __fadd_rn(__fmul_rn(a.c_mean0, x0), __fmul_rn(a.c_mean1, second));
            if (a.c_noise != 0.0f) v = __fadd_rn(v, __fmul_rn(a.c_noise, zs[j]));       // :326/:328
            o[j] = v;
        }
        reinterpret_cast<float4*>(a.x)[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

static int grid_for(int64_t n4) { return (int)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256); }

int launch_sampler_update(int kind, float* x, const float* eps, const float* noise, float c_x0a, float c_x0b,
                          float c_mean0, float c_mean1, float c_noise, int clip, int64_t n, int use_philox,
                          uint64_t seed, uint64_t sample_offset, uint64_t draw, int64_t per_sample, hipStream_t s) {
    MCVD_REQUIRE(n % 4 == 0 && (per_sample % 4 == 0 || !use_philox), "sampler_update: n must be a multiple of 4");
    MCVD_REQUIRE(c_noise == 0.0f || use_philox || noise, "sampler_update: noise needed");
    UpdArgs a{kind, x, eps, noise, c_x0a, c_x0b, c_mean0, c_mean1, c_noise, clip, n, use_philox, seed, sample_offset, draw,
              per_sample};
    hipLaunchKernelGGL(sampler_update_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, a);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// x = ca*x + cb*z      (t_min re-noise, models/__init__.py:279)
__global__ __launch_bounds__(256) void renoise_kernel(float* x, const float* noise, float ca, float cb, int64_t n,
                                                       int use_philox, uint64_t seed, uint64_t sample_offset,
                                                       uint64_t draw, int64_t per_sample) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 xv = reinterpret_cast<float4*>(x)[i];
        float4 zv;
        if (use_philox) {
            const int64_t e = i * 4;
            const int64_t row = e / per_sample;
            zv = philox_normal4(seed, sample_offset + (uint64_t)row, draw, (uint64_t)((e - row * per_sample) >> 2));
        } else {
            zv = reinterpret_cast<const float4*>(noise)[i];
        }
        xv.x = __fadd_rn(__fmul_rn(ca, xv.x), __fmul_rn(cb, zv.x));
        xv.y = __fadd_rn(__fmul_rn(ca, xv.y), __fmul_rn(cb, zv.y));
        xv.z = __fadd_rn(__fmul_rn(ca, xv.z), __fmul_rn(cb, zv.z));
        xv.w = __fadd_rn(__fmul_rn(ca, xv.w), __fmul_rn(cb, zv.w));
        reinterpret_cast<float4*>(x)[i] = xv;
    }
}

int launch_renoise(float* x, const float* noise, float ca, float cb, int64_t n, int use_philox, uint64_t seed,
                   uint64_t sample_offset, uint64_t draw, int64_t per_sample, hipStream_t s) {
    MCVD_REQUIRE(n % 4 == 0, "renoise: n must be a multiple of 4");
    MCVD_REQUIRE(use_philox || noise, "renoise: noise needed");
    hipLaunchKernelGGL(renoise_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, x, noise, ca, cb, n, use_philox, seed,
                       sample_offset, draw, per_sample);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// x = x - c*eps       (denoise, models/__init__.py:333)
__global__ __launch_bounds__(256) void axpy_out_kernel(float* x, const float* eps, float c, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 xv = reinterpret_cast<float4*>(x)[i];
        const float4 ev = reinterpret_cast<const float4*>(eps)[i];
        xv.x = __fsub_rn(xv.x, __fmul_rn(c, ev.x));
        xv.y = __fsub_rn(xv.y, __fmul_rn(c, ev.y));
        xv.z = __fsub_rn(xv.z, __fmul_rn(c, ev.z));
        xv.w = __fsub_rn(xv.w, __fmul_rn(c, ev.w));
        reinterpret_cast<float4*>(x)[i] = xv;
    }
}

int launch_axpy_out(float* x, const float* eps, float c, int64_t n, hipStream_t s) {
    MCVD_REQUIRE(n % 4 == 0, "axpy: n must be a multiple of 4");
    hipLaunchKernelGGL(axpy_out_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, x, eps, c, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- classifier-free guidance.  A guided step is ONE forward at 2B rows -- rows [0, B) on (x, cond), rows [B, 2B) on (x, cond_weak) --
// and one of the kernels below, which forms, per element, in fp32 with one rounding per operation and no fma (as torch evaluates
// `e_c + (s - 1) * (e_c - e_u)`),
//     d = e_c - e_u;   e = e_c + w * d            w = float32(s - 1)
// and then runs the chain of its unguided twin above on e: same operations, same order.  n, per_sample and the Philox row are those of
// the B-row call; `xdup` (NULL, or the network's [2B] input buffer) receives the new x in both halves in the same pass.
__device__ __forceinline__ float guided_eps(float ec, float eu, float w) { return __fadd_rn(ec, __fmul_rn(w, __fsub_rn(ec, eu))); }

__device__ __forceinline__ void store_dup(float* xdup, int64_t i, int64_t n4, float4 v) {
    reinterpret_cast<float4*>(xdup)[i] = v;
    reinterpret_cast<float4*>(xdup)[n4 + i] = v;
}

struct GuidedUpdArgs {
    UpdArgs u;              // u.eps = the conditional half
    const float* eps_u;     // the weak half
    float* xdup;
    float w;
};

__global__ __launch_bounds__(256) void sampler_update_guided_kernel(GuidedUpdArgs g) {
    const UpdArgs& a = g.u;
    const int64_t n4 = a.n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
        const float4 cv = reinterpret_cast<const float4*>(a.eps)[i];
        const float4 uv = reinterpret_cast<const float4*>(g.eps_u)[i];
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.c_noise != 0.0f) {
            if (a.use_philox) {
                const int64_t e = i * 4;
                const int64_t row = e / a.per_sample;             // a row of the B-row call
                zv = philox_normal4(a.seed, a.sample_offset + (uint64_t)row, a.draw, (uint64_t)((e - row * a.per_sample) >> 2));
            } else {
                zv = reinterpret_cast<const float4*>(a.noise)[i];
            }
        }
        float xs[4] = {xv.x, xv.y, xv.z, xv.w}, cs[4] = {cv.x, cv.y, cv.z, cv.w}, us[4] = {uv.x, uv.y, uv.z, uv.w};
        float zs[4] = {zv.x, zv.y, zv.z, zv.w}, o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ej = guided_eps(cs[j], us[j], g.w);
            float x0 = __fmul_rn(a.c_x0a, __fsub_rn(xs[j], __fmul_rn(a.c_x0b, ej)));
            if (a.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
            const float second = (a.kind == 0) ? xs[j] : ej;
            float v = __fadd_rn(__fmul_rn(a.c_mean0, x0), __fmul_rn(a.c_mean1, second));
            if (a.c_noise != 0.0f) v = __fadd_rn(v, __fmul_rn(a.c_noise, zs[j]));
            o[j] = v;
        }
        const float4 ov = make_float4(o[0], o[1], o[2], o[3]);
        reinterpret_cast<float4*>(a.x)[i] = ov;
        if (g.xdup) store_dup(g.xdup, i, n4, ov);
    }
}

int launch_sampler_update_guided(int kind, float* x, float* xdup, const float* eps_c, const float* eps_u, const float* noise, float w,
                                 float c_x0a, float c_x0b, float c_mean0, float c_mean1, float c_noise, int clip, int64_t n,
                                 int use_philox, uint64_t seed, uint64_t sample_offset, uint64_t draw, int64_t per_sample,
                                 hipStream_t s) {
    MCVD_REQUIRE(x && eps_c && eps_u, "sampler_update_guided: NULL argument");
    MCVD_REQUIRE(n % 4 == 0 && (per_sample % 4 == 0 || !use_philox), "sampler_update_guided: n must be a multiple of 4");
    MCVD_REQUIRE(c_noise == 0.0f || use_philox || noise, "sampler_update_guided: noise needed");
    GuidedUpdArgs g{{kind, x, eps_c, noise, c_x0a, c_x0b, c_mean0, c_mean1, c_noise, clip, n, use_philox, seed, sample_offset, draw,
                     per_sample}, eps_u, xdup, w};
    hipLaunchKernelGGL(sampler_update_guided_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, g);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// eps_out = e  (the host loops and F-PNDM, whose lincomb / transfer kernels then run on B rows)
__global__ __launch_bounds__(256) void guidance_combine_kernel(float* out, const float* eps_c, const float* eps_u, float w, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 c = reinterpret_cast<const float4*>(eps_c)[i];
        const float4 u = reinterpret_cast<const float4*>(eps_u)[i];
        reinterpret_cast<float4*>(out)[i] =
            make_float4(guided_eps(c.x, u.x, w), guided_eps(c.y, u.y, w), guided_eps(c.z, u.z, w), guided_eps(c.w, u.w, w));
    }
}

int launch_guidance_combine(float* out, const float* eps_c, const float* eps_u, float w, int64_t n, hipStream_t s) {
    MCVD_REQUIRE(out && eps_c && eps_u && n % 4 == 0, "guidance_combine: NULL argument, or n is not a multiple of 4");
    hipLaunchKernelGGL(guidance_combine_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, out, eps_c, eps_u, w, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// x = x - c*e         (the guided denoise pass; nothing reads the network's input buffer afterwards)
__global__ __launch_bounds__(256) void axpy_out_guided_kernel(float* x, const float* eps_c, const float* eps_u, float w, float c,
                                                               int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 xv = reinterpret_cast<float4*>(x)[i];
        const float4 cv = reinterpret_cast<const float4*>(eps_c)[i];
        const float4 uv = reinterpret_cast<const float4*>(eps_u)[i];
        xv.x = __fsub_rn(xv.x, __fmul_rn(c, guided_eps(cv.x, uv.x, w)));
        xv.y = __fsub_rn(xv.y, __fmul_rn(c, guided_eps(cv.y, uv.y, w)));
        xv.z = __fsub_rn(xv.z, __fmul_rn(c, guided_eps(cv.z, uv.z, w)));
        xv.w = __fsub_rn(xv.w, __fmul_rn(c, guided_eps(cv.w, uv.w, w)));
        reinterpret_cast<float4*>(x)[i] = xv;
    }
}

int launch_axpy_out_guided(float* x, const float* eps_c, const float* eps_u, float w, float c, int64_t n, hipStream_t s) {
    MCVD_REQUIRE(x && eps_c && eps_u && n % 4 == 0, "axpy_guided: NULL argument, or n is not a multiple of 4");
    hipLaunchKernelGGL(axpy_out_guided_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, x, eps_c, eps_u, w, c, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// x = ca*x + cb*z     (the t_min re-noise of a guided call: the B rows draw what an unguided call draws; both halves of xdup get the result)
__global__ __launch_bounds__(256) void renoise_dup_kernel(float* x, float* xdup, const float* noise, float ca, float cb, int64_t n,
                                                           int use_philox, uint64_t seed, uint64_t sample_offset, uint64_t draw,
                                                           int64_t per_sample) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 xv = reinterpret_cast<float4*>(x)[i];
        float4 zv;
        if (use_philox) {
            const int64_t e = i * 4;
            const int64_t row = e / per_sample;
            zv = philox_normal4(seed, sample_offset + (uint64_t)row, draw, (uint64_t)((e - row * per_sample) >> 2));
        } else {
            zv = reinterpret_cast<const float4*>(noise)[i];
        }
        xv.x = __fadd_rn(__fmul_rn(ca, xv.x), __fmul_rn(cb, zv.x));
        xv.y = __fadd_rn(__fmul_rn(ca, xv.y), __fmul_rn(cb, zv.y));
        xv.z = __fadd_rn(__fmul_rn(ca, xv.z), __fmul_rn(cb, zv.z));
        xv.w = __fadd_rn(__fmul_rn(ca, xv.w), __fmul_rn(cb, zv.w));
        reinterpret_cast<float4*>(x)[i] = xv;
        store_dup(xdup, i, n4, xv);
    }
}

int launch_renoise_dup(float* x, float* xdup, const float* noise, float ca, float cb, int64_t n, int use_philox, uint64_t seed,
                       uint64_t sample_offset, uint64_t draw, int64_t per_sample, hipStream_t s) {
    MCVD_REQUIRE(x && xdup && n % 4 == 0 && (per_sample % 4 == 0 || !use_philox), "renoise_dup: NULL argument, or n is not a multiple of 4");
    MCVD_REQUIRE(use_philox || noise, "renoise_dup: noise needed");
    hipLaunchKernelGGL(renoise_dup_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, x, xdup, noise, ca, cb, n, use_philox, seed,
                       sample_offset, draw, per_sample);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// f16x2 range guard: the two-piece fp16 kernels clamp nothing -- an activation beyond the fp16 range becomes Inf, the accumulators NaN,
// GroupNorm spreads it over the sample -- so a scan of the forward's epsilon sees every overflow.  One flag word, written only on a hit.
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const float* v, int64_t n, int* flag) {
    const int64_t n4 = n >> 2;
    bool bad = false;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 e = reinterpret_cast<const float4*>(v)[i];
        // exponent all ones <=> Inf or NaN
        bad |= ((__float_as_uint(e.x) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(e.y) & 0x7f800000u) == 0x7f800000u) |
               ((__float_as_uint(e.z) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(e.w) & 0x7f800000u) == 0x7f800000u);
    }
    if (bad) *flag = 1;
}

int launch_nonfinite_flag(const float* v, int64_t n, int* flag, hipStream_t s) {
    MCVD_REQUIRE(n % 4 == 0 && flag, "nonfinite_flag: n must be a multiple of 4");
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, v, n, flag);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- F-PNDM pieces (models/pndm.py).  One rounding per operation, in the order of the reference's tensor expressions, so the
// multistep combination is bit-identical to torch's elementwise evaluation: plain operators under `fp contract(off)` (the
// __fmul_rn / __fadd_rn device functions are inlined with the translation unit's default contraction and DO get fused).
struct LinArgs {
    const float* in[4];
    float w[4];
    float scale;
    int nin;
};

// out = scale * (((w0*in0 + w1*in1) + w2*in2) + w3*in3)     runge_kutta :15, gen_order_4 :47
__global__ __launch_bounds__(256) void lincomb_kernel(float* out, LinArgs a, int64_t n) {
#pragma clang fp contract(off)
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float t = a.w[0] * a.in[0][i];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (k < a.nin) {
                const float p = a.w[k] * a.in[k][i];
                t = t + p;
            }
        out[i] = a.scale * t;
    }
}

int launch_lincomb(float* out, const float* const* in, const float* w, float scale, int nin, int64_t n, hipStream_t s) {
    LinArgs a{};
    for (int k = 0; k < 4; ++k) { a.in[k] = k < nin ? in[k] : in[0]; a.w[k] = k < nin ? w[k] : 0.0f; }
    a.scale = scale;
    a.nin = nin;
    hipLaunchKernelGGL(lincomb_kernel, dim3(grid_for(n)), dim3(256), 0, s, out, a, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// x_next = clip?( x + d * (c1 * x - c2 * e) )               transfer :19-33
__global__ __launch_bounds__(256) void pndm_transfer_kernel(float* out, const float* x, const float* e, float d, float c1,
                                                             float c2, int clip, int64_t n) {
#pragma clang fp contract(off)
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float xv = x[i];
        const float p = c1 * xv, q = c2 * e[i];
        const float r = p - q;
        const float dr = d * r;
        float v = xv + dr;
        if (clip) v = fminf(fmaxf(v, -1.0f), 1.0f);
        out[i] = v;
    }
}

int launch_pndm_transfer(float* out, const float* x, const float* e, float d, float c1, float c2, int clip, int64_t n,
                         hipStream_t s) {
    hipLaunchKernelGGL(pndm_transfer_kernel, dim3(grid_for(n)), dim3(256), 0, s, out, x, e, d, c1, c2, clip, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void randn_kernel(float* out, uint64_t seed, uint64_t sample_offset, uint64_t draw,
                                                     int64_t n, int64_t per_sample) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * 4;
        const int64_t row = e / per_sample;
        reinterpret_cast<float4*>(out)[i] =
            philox_normal4(seed, sample_offset + (uint64_t)row, draw, (uint64_t)((e - row * per_sample) >> 2));
    }
}

int launch_randn(float* out, uint64_t seed, uint64_t sample_offset, uint64_t draw, int B, int64_t per_sample,
                 hipStream_t s) {
    MCVD_REQUIRE(per_sample % 4 == 0, "randn: per_sample must be a multiple of 4");
    const int64_t n = (int64_t)B * per_sample;
    hipLaunchKernelGGL(randn_kernel, dim3(grid_for(n >> 2)), dim3(256), 0, s, out, seed, sample_offset, draw, n, per_sample);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mcvd
