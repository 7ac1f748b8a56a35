// The FID InceptionV3 (evaluation/inception.py: InceptionV3 :16-163, fid_inception_v3 :184-208, the patched blocks :211-328) on the device:
// the detector of fast_fid, fid_pr and nearest_neighbors.  The weights come from the caller (mcvd_inception_set_param, by the key names of
// pt_inception-2015-12-05-6726825d.pth); the package holds none.
//
//   x    = F.interpolate(images, (299, 299), bilinear, align_corners=False); 2 x - 1     inception_prep_kernel: per-axis tables from the host
//                                                                                        (fvd.cpp's coordinate rule and lerp order), any H, W
//   94 x   BasicConv2d = conv (no bias) + BatchNorm(eps 0.001, eval) + ReLU              the detector nets' conv (detector_ops.h): relu(fma(acc,
//                                                                                        alpha, beta)), alpha = w / sqrt(var + 0.001),
//                                                                                        beta = b - mean alpha formed in fp64 on the host
//                                                                                        and rounded once; K chunks of 32 rows
//   torch.cat of a block's branches                                                      no pass: every branch stores its channel slice
//   F.avg_pool2d(3, 1, 1, count_include_pad=False), F.max_pool2d(3, 1, 1)                launch_pool3 (detector_ops.h)
//   MaxPool2d(3, 2)                                                                      launch_maxpool3s2
//   AdaptiveAvgPool2d((1, 1))                                                            launch_global_avg: fp64 sum in index order
//
// The conv, the pools and the host scaffold of the net (parameter blob, workspace, per-size tables) live in kernels/detector_ops.cpp and
// are LPIPS's too; this file keeps the prep kernel, the Program (the net as a list of ops) and the net.
// Everything runs on the context's stream; nothing reads the environment.
#include "../inception.h"
#include "../model.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace mcvd {
namespace {

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

void inception_axis_table(int S, std::vector<int>& tab) {
    constexpr int O = INCEPTION_SIZE;
    tab.assign(4 * O, 0);
    std::vector<float> l(2 * O);
    bilinear_axis_table(S, O, &tab[0], &tab[O], &l[0], &l[O]);
    memcpy(&tab[2 * O], l.data(), 2 * O * sizeof(float));
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

static ConvGeom geom(const IncLayer& L) { return {L.Cin, L.Cout, L.kh, L.kw}; }

int inception_finalize(mcvd_inception* n) {
    const std::vector<IncLayer>& LS = program().layers;
    const int NL = (int)LS.size();
    for (int i = 0; i < NL; ++i) {
        const char* missing = n->w[i].empty() ? ".conv.weight" : n->bn_w[i].empty() ? ".bn.weight" : n->bn_b[i].empty() ? ".bn.bias"
                              : n->bn_m[i].empty() ? ".bn.running_mean" : n->bn_v[i].empty() ? ".bn.running_var" : nullptr;
        if (missing) { set_error("inception_finalize: missing %s%s", LS[i].name.c_str(), missing); return MCVD_ESTATE; }
    }
    size_t total = 0, raw_max = 0;
    for (int i = 0; i < NL; ++i) {
        total += ParamBlob::floats_needed(geom(LS[i]));
        raw_max = std::max(raw_max, n->w[i].size());
    }
    ParamBlob blob(n->ctx->stream, "inception_finalize");
    if (int rc = blob.begin(&n->params, total, raw_max)) return rc;
    std::vector<float> al, be;
    for (int i = 0; i < NL; ++i) {
        const IncLayer& L = LS[i];
        al.resize(L.Cout);
        be.resize(L.Cout);
        for (int c = 0; c < L.Cout; ++c) {      // fp64, rounded once each
            const double a64 = (double)n->bn_w[i][c] / sqrt((double)n->bn_v[i][c] + 0.001);
            al[c] = (float)a64;
            be[c] = (float)((double)n->bn_b[i][c] - (double)n->bn_m[i][c] * a64);
        }
        if (int rc = blob.conv(geom(L), n->w[i].data(), al.data(), be.data(), &n->conv[i])) return rc;
    }
    n->finalized = true;
    return 0;
}

static int build_axis_table(int S, std::vector<int>& tab) {
    inception_axis_table(S, tab);
    return 0;
}

static int axis_tab(mcvd_inception* n, int in_size, const int** tab) {
    const TableCache::Entry* e;
    if (int rc = n->axis.get(in_size, build_axis_table, n->ctx->stream, &e)) return rc;
    *tab = e->dev;
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
    if (int rc = grow((void**)&n->ws, &n->ws_bytes, (size_t)P.total * cap * sizeof(float), s)) return rc;
    const int *tab_h, *tab_w;
    if (int rc = axis_tab(n, H, &tab_h)) return rc;
    if (int rc = axis_tab(n, W, &tab_w)) return rc;
    const long long wcap = cap;      // the layout of this call; a workspace left larger by an earlier call holds it as well

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
                const ConvParams& cv = n->conv[op.layer];
                rc = launch_conv(x, cv.wp, cv.tab, cv.alpha, cv.beta, y, nimg, L.Cin, op.H, op.W, L.Cout, L.kh, L.kw, L.stride, L.ph, L.pw, 1, op.c0,
                                 op.Cdst, "inception_forward", s);
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
    conv.resize(nl);
}

mcvd_inception::~mcvd_inception() {
    if (params) (void)hipFree(params);
    if (ws) (void)hipFree(ws);
}
