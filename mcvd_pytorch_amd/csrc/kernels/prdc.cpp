// Improved precision and recall (k-nearest-neighbour manifolds) of fast_fid, evaluation/fid_PR.py:209-259, without the pairwise matrices.
//
// knn_radii:     radii2[i] = the (k+1)-th smallest squared distance from row i to all rows of the same matrix, itself included
//                (cdist(X, X).kthvalue(k + 1).values ** 2, :251).
// manifold_hits: hit[i] = 1 iff some ref row j has dist2(query_i, ref_j) <= ref_radii2[j]  ((dist <= NNk).any(dim=1), :256, :258).
//
// Both are one sweep over a Gram matrix that is never stored.  The rows whose result is wanted ("owners") sit on the column axis of
// v_mfma_f64_16x16x4_f64 and the rows they are compared with ("swept") on its row axis: lane l supplies A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15]; result register v of lane l is C[row (l >> 4) + 4 v][col l & 15] -- so a lane keeps ONE owner (l & 15) for the
// whole sweep and holds that owner's state in registers: the sorted list of its PD_L smallest squared distances (radii), or an OR-ed flag
// (hits).  For the radii X x X is symmetric, so owners as columns are as good as rows; for the hits the product is ref x query.
//
// A workgroup of four waves owns 64 owners (16 per wave) and a range of 64-row swept tiles; per tile every wave accumulates four 16 x 16
// blocks over d in chunks of PD_KC feature columns that the workgroup stages in LDS as fp64, k-major (the next chunk is fetched into
// registers while the current one is multiplied).  When a tile's d is done: d2 = max(0, (|a|^2 + |b|^2) - 2 a.b) with the row norms of a
// first small kernel, and the list insertion or the comparison.  At the end the four lanes that share an owner exchange their state with
// two wave shuffles (xor 16, xor 32) -- a change from a merge through LDS: the lists are eight registers and need no barrier this way.
//
// The swept axis is split over workgroups (blockIdx.y) by pd_plan, a rule of the two row counts alone; each split writes its owners' partial
// lists [split][owner][PD_L] or flags [split][owner], and a second small launch merges them in split order.  Selecting the smallest
// values of a multiset and OR are order-independent, so the results are bit-identical run to run AND independent of the split.
// Everything is written with ordinary vector stores.
#include "../common.h"

namespace mcvd {
namespace {

constexpr int PD_T = 64;                    // rows of a tile, on both axes
constexpr int PD_KC = 32;                   // feature columns per staged chunk
constexpr int PD_LD = PD_T + 1;             // LDS stride between two feature columns (doubles): staging stores spread over the banks
constexpr int PD_THREADS = 256;
constexpr int PD_L = 8;                     // list length per owner: k + 1 <= 8
constexpr int PD_BLOCKS = 512;              // workgroups the split rule aims at (two per compute unit)
constexpr int PD_MAX_SPLITS = 256;

__device__ __forceinline__ double pd_load(const void* x, int is64, int64_t i) {
    return is64 ? static_cast<const double*>(x)[i] : (double)static_cast<const float*>(x)[i];
}

// v into the ascending list (a multiset: equal values are kept as often as they come)
__device__ __forceinline__ void pd_insert(double (&best)[PD_L], double v) {
    if (v < best[PD_L - 1]) {
#pragma unroll
        for (int i = 0; i < PD_L; ++i) {
            const double lo = fmin(v, best[i]);
            v = fmax(v, best[i]);
            best[i] = lo;
        }
    }
}

// out[r] = sum of squares of row r: one wave per row, lane partials in column order, then an xor butterfly (the same value in every lane)
__global__ __launch_bounds__(PD_THREADS) void pd_norms_kernel(const void* __restrict__ x, int is64, int64_t ld, int n, int d,
                                                                double* __restrict__ out) {
    const int row = blockIdx.x * (PD_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double s = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double v = pd_load(x, is64, (int64_t)row * ld + c);
        s = fma(v, v, s);
    }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[row] = s;
}

struct PdArgs {
    const void* a;                          // swept rows [na, d]
    const void* b;                          // owner rows [nb, d]
    int a64, b64;
    int64_t lda, ldb;
    int na, nb, d;
    int tiles_per_split;
    const double* norm_a;                   // [na]
    const double* norm_b;                   // [nb]
    const double* radii_a;                  // hits: squared radius of every swept row
    double* part_list;                      // radii: [splits, nb, PD_L]
    uint8_t* part_hit;                      // hits:  [splits, nb]
};

template <int HITS>
__global__ __launch_bounds__(PD_THREADS) void pd_sweep_kernel(PdArgs p) {
    __shared__ double As[PD_KC * PD_LD];
    __shared__ double Bs[PD_KC * PD_LD];
    typedef double double4_t __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lc = lane & 15, lk = lane >> 4;
    const int c0 = blockIdx.x * PD_T;
    const int ntile = (p.na + PD_T - 1) / PD_T;
    const int t0 = blockIdx.y * p.tiles_per_split;
    const int t1 = min(ntile, t0 + p.tiles_per_split);
    const int nk = (p.d + PD_KC - 1) / PD_KC;
    const int nit = (t1 - t0) * nk;
    const int ck = tid & (PD_KC - 1), cr = tid / PD_KC;          // staging: feature column ck of the chunk, rows cr, cr + 8, ...
    constexpr int PD_ROWS = PD_T * PD_KC / PD_THREADS;           // rows of either tile a thread stages per chunk

    double ra[PD_ROWS], rb[PD_ROWS];
    auto fetch = [&](int it) {
        const int r0 = (t0 + it / nk) * PD_T;
        const int k = (it % nk) * PD_KC + ck;
        const bool kin = k < p.d;
#pragma unroll
        for (int j = 0; j < PD_ROWS; ++j) {
            const int r = r0 + cr + (PD_THREADS / PD_KC) * j, c = c0 + cr + (PD_THREADS / PD_KC) * j;
            ra[j] = (kin && r < p.na) ? pd_load(p.a, p.a64, (int64_t)r * p.lda + k) : 0.0;
            rb[j] = (kin && c < p.nb) ? pd_load(p.b, p.b64, (int64_t)c * p.ldb + k) : 0.0;
        }
    };

    const int col = c0 + w * 16 + lc;                            // this lane's owner
    const bool cin = col < p.nb;
    const double nbv = cin ? p.norm_b[col] : 0.0;
    double best[PD_L];
#pragma unroll
    for (int i = 0; i < PD_L; ++i) best[i] = INFINITY;
    int hit = 0;
    double4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};

    fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();                                         // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < PD_ROWS; ++j) {
            As[ck * PD_LD + cr + (PD_THREADS / PD_KC) * j] = ra[j];
            Bs[ck * PD_LD + cr + (PD_THREADS / PD_KC) * j] = rb[j];
        }
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
#pragma unroll
        for (int s = 0; s < PD_KC / 4; ++s) {
            const int kk = 4 * s + lk;
            const double b = Bs[kk * PD_LD + w * 16 + lc];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[kk * PD_LD + 16 * t + lc], b, acc[t], 0, 0, 0);
        }
        if ((it + 1) % nk == 0) {                                // the tile's d is complete
            const int r0 = (t0 + it / nk) * PD_T;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = r0 + 16 * t + lk + 4 * v;
                    if (cin && r < p.na) {
                        const double d2 = fmax(0.0, (p.norm_a[r] + nbv) - 2.0 * acc[t][v]);
                        if (HITS)
                            hit |= d2 <= p.radii_a[r] ? 1 : 0;
                        else
                            pd_insert(best, d2);
                    }
                }
                acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
            }
        }
    }

    // the four lanes of an owner: lanes lc, lc + 16, lc + 32, lc + 48 of the wave
    if (HITS) {
        hit |= __shfl_xor(hit, 16);
        hit |= __shfl_xor(hit, 32);
        if (lk == 0 && cin) p.part_hit[(int64_t)blockIdx.y * p.nb + col] = (uint8_t)hit;
    } else {
        for (int o = 16; o <= 32; o <<= 1) {
            double other[PD_L];
#pragma unroll
            for (int i = 0; i < PD_L; ++i) other[i] = __shfl_xor(best[i], o);
#pragma unroll
            for (int i = 0; i < PD_L; ++i) pd_insert(best, other[i]);
        }
        if (lk == 0 && cin) {
            double* dst = p.part_list + ((int64_t)blockIdx.y * p.nb + col) * PD_L;
#pragma unroll
            for (int i = 0; i < PD_L; ++i) dst[i] = best[i];
        }
    }
}

// radii2[c] = element k (0-based) of the merged ascending list of owner c, the splits taken in index order
__global__ __launch_bounds__(PD_THREADS) void pd_merge_radii_kernel(const double* __restrict__ part, int splits, int nb, int k,
                                                                      double* __restrict__ radii2) {
    const int c = blockIdx.x * PD_THREADS + threadIdx.x;
    if (c >= nb) return;
    double best[PD_L];
#pragma unroll
    for (int i = 0; i < PD_L; ++i) best[i] = INFINITY;
    for (int s = 0; s < splits; ++s) {
        const double* src = part + ((int64_t)s * nb + c) * PD_L;
#pragma unroll
        for (int i = 0; i < PD_L; ++i) pd_insert(best, src[i]);
    }
    double r = best[0];
#pragma unroll
    for (int i = 1; i < PD_L; ++i) r = i == k ? best[i] : r;
    radii2[c] = r;
}

__global__ __launch_bounds__(PD_THREADS) void pd_merge_hits_kernel(const uint8_t* __restrict__ part, int splits, int nb, uint8_t* __restrict__ hit) {
    const int c = blockIdx.x * PD_THREADS + threadIdx.x;
    if (c >= nb) return;
    int h = 0;
    for (int s = 0; s < splits; ++s) h |= part[(int64_t)s * nb + c];
    hit[c] = (uint8_t)(h ? 1 : 0);
}

struct PdPlan {
    int colblocks;                          // workgroups along the owners
    int tiles;                              // 64-row tiles of the swept axis
    int tiles_per_split;
    int splits;                             // workgroups along the swept axis; every split has at least one tile
};

// The split rule, of (swept rows, owner rows) alone: enough splits for about PD_BLOCKS workgroups, never more than tiles or PD_MAX_SPLITS
PdPlan pd_plan(int na, int nb) {
    PdPlan pl;
    pl.colblocks = (nb + PD_T - 1) / PD_T;
    pl.tiles = (na + PD_T - 1) / PD_T;
    int want = (PD_BLOCKS + pl.colblocks - 1) / pl.colblocks;
    if (want > pl.tiles) want = pl.tiles;
    if (want > PD_MAX_SPLITS) want = PD_MAX_SPLITS;
    if (want < 1) want = 1;
    pl.tiles_per_split = (pl.tiles + want - 1) / want;
    pl.splits = (pl.tiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
    return pl;
}

int64_t pd_align8(int64_t bytes) { return (bytes + 7) / 8 * 8; }

int pd_norms(const void* x, int is64, int64_t ld, int n, int d, double* out, hipStream_t s) {
    const int per = PD_THREADS / 64;
    hipLaunchKernelGGL(pd_norms_kernel, dim3((n + per - 1) / per), dim3(PD_THREADS), 0, s, x, is64, ld, n, d, out);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int64_t knn_radii_scratch_bytes(int n) {
    const PdPlan pl = pd_plan(n, n);
    return (int64_t)n * sizeof(double) + (int64_t)pl.splits * n * PD_L * (int64_t)sizeof(double);
}

int64_t manifold_hits_scratch_bytes(int nq, int nr) {
    const PdPlan pl = pd_plan(nr, nq);
    return ((int64_t)nq + nr) * sizeof(double) + pd_align8((int64_t)pl.splits * nq);
}

int launch_knn_radii(const void* x, int is64, int64_t ld, int n, int d, int k, double* radii2, void* scratch, hipStream_t s) {
    MCVD_REQUIRE(x && radii2 && scratch, "knn_radii: NULL argument");
    MCVD_REQUIRE(k >= 1 && k <= PD_L - 1, "knn_radii: k = %d is outside 1..%d", k, PD_L - 1);
    MCVD_REQUIRE(n >= k + 1 && n < (1 << 24), "knn_radii: %d rows (at least k + 1 = %d: kthvalue raises below that; fewer than 2^24)", n, k + 1);
    MCVD_REQUIRE(d >= 1 && d <= 2048 && ld >= d, "knn_radii: bad d = %d (1 to 2048) or leading dimension %lld", d, (long long)ld);
    const PdPlan pl = pd_plan(n, n);
    double* norms = static_cast<double*>(scratch);
    if (int rc = pd_norms(x, is64, ld, n, d, norms, s)) return rc;
    PdArgs p;
    p.a = p.b = x;
    p.a64 = p.b64 = is64;
    p.lda = p.ldb = ld;
    p.na = p.nb = n;
    p.d = d;
    p.tiles_per_split = pl.tiles_per_split;
    p.norm_a = p.norm_b = norms;
    p.radii_a = nullptr;
    p.part_list = norms + n;
    p.part_hit = nullptr;
    hipLaunchKernelGGL(pd_sweep_kernel<0>, dim3(pl.colblocks, pl.splits), dim3(PD_THREADS), 0, s, p);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pd_merge_radii_kernel, dim3((n + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, s, p.part_list, pl.splits, n, k, radii2);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_manifold_hits(const void* q, int q64, int64_t ldq, int nq, const void* r, int r64, int64_t ldr, int nr, int d, const double* ref_radii2,
                         uint8_t* hit, void* scratch, hipStream_t s) {
    MCVD_REQUIRE(q && r && ref_radii2 && hit && scratch, "manifold_hits: NULL argument");
    MCVD_REQUIRE(nq >= 1 && nq < (1 << 24) && nr >= 1 && nr < (1 << 24), "manifold_hits: %d query and %d ref rows (1 to 2^24 - 1 each)", nq, nr);
    MCVD_REQUIRE(d >= 1 && d <= 2048 && ldq >= d && ldr >= d, "manifold_hits: bad d = %d (1 to 2048) or leading dimensions %lld, %lld", d,
                 (long long)ldq, (long long)ldr);
    const PdPlan pl = pd_plan(nr, nq);
    double* norm_q = static_cast<double*>(scratch);
    double* norm_r = norm_q + nq;
    if (int rc = pd_norms(q, q64, ldq, nq, d, norm_q, s)) return rc;
    if (int rc = pd_norms(r, r64, ldr, nr, d, norm_r, s)) return rc;
    PdArgs p;
    p.a = r;
    p.b = q;
    p.a64 = r64;
    p.b64 = q64;
    p.lda = ldr;
    p.ldb = ldq;
    p.na = nr;
    p.nb = nq;
    p.d = d;
    p.tiles_per_split = pl.tiles_per_split;
    p.norm_a = norm_r;
    p.norm_b = norm_q;
    p.radii_a = ref_radii2;
    p.part_list = nullptr;
    p.part_hit = reinterpret_cast<uint8_t*>(norm_r + nr);
    hipLaunchKernelGGL(pd_sweep_kernel<1>, dim3(pl.colblocks, pl.splits), dim3(PD_THREADS), 0, s, p);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pd_merge_hits_kernel, dim3((nq + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, s, p.part_hit, pl.splits, nq, hit);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- nearest neighbours of samples in a data set (evaluation/nearest_neighbor.py:70-114) ---------------------------------------------
//
// knn_search: the same sweep with the queries as owners and the data rows swept, carrying indices.  A lane keeps its query's NN_L = 16
// best (d2, row) pairs in registers, ascending under the total order (d2, row) -- equal d2: lower row first.  With a second view of the
// queries (the mirrored samples) both views are multiplied against the SAME staged data chunk, one LDS read of it feeding two matrix
// instructions, and a pair's d2 is the smaller of the two.  A pair's d2 depends on its two rows alone (norms from the small kernel, one
// accumulation order over d), never on the tile, the split or the call it falls in: the k smallest of a union of pieces are the k
// smallest of the whole, bit for bit.  Rows inside a call are 32-bit; the merge launch adds index_base and, with `merge`, takes the
// caller's earlier lists in as well.
namespace {

constexpr int NN_L = 16;                    // list length per query: k <= 16 (the first k of the 16 best are the k best)
constexpr int NN_NONE = 0x7fffffff;         // row of an empty slot: behind every real row at d2 = +inf

template <typename I>
__device__ __forceinline__ bool nn_less(double v, I i, double w, I j) {
    return v < w || (v == w && i < j);      // NaN compares false both ways: never selected
}

template <typename I>
__device__ __forceinline__ void nn_insert(double (&bv)[NN_L], I (&bi)[NN_L], double v, I i) {
    if (nn_less(v, i, bv[NN_L - 1], bi[NN_L - 1])) {
#pragma unroll
        for (int j = 0; j < NN_L; ++j) {
            const bool lt = nn_less(v, i, bv[j], bi[j]);
            const double tv = lt ? bv[j] : v;
            const I ti = lt ? bi[j] : i;
            bv[j] = lt ? v : bv[j];
            bi[j] = lt ? i : bi[j];
            v = tv;
            i = ti;
        }
    }
}

struct NnArgs {
    const void* a;                          // swept data rows [na, d]
    const void* b;                          // queries [nb, d]
    const void* b2;                         // second view of the queries (VIEWS == 2)
    int a64, b64, b264;
    int64_t lda, ldb, ldb2;
    int na, nb, d;
    int tiles_per_split;
    const double* norm_a;                   // [na]
    const double* norm_b;                   // [nb]
    const double* norm_b2;                  // [nb]
    double* part_d2;                        // [splits, nb, NN_L]
    int* part_row;                          // [splits, nb, NN_L]
};

template <int VIEWS>
__global__ __launch_bounds__(PD_THREADS) void nn_sweep_kernel(NnArgs p) {
    __shared__ double As[PD_KC * PD_LD];
    __shared__ double Bs[VIEWS][PD_KC * PD_LD];
    typedef double double4_t __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lc = lane & 15, lk = lane >> 4;
    const int c0 = blockIdx.x * PD_T;
    const int ntile = (p.na + PD_T - 1) / PD_T;
    const int t0 = blockIdx.y * p.tiles_per_split;
    const int t1 = min(ntile, t0 + p.tiles_per_split);
    const int nk = (p.d + PD_KC - 1) / PD_KC;
    const int nit = (t1 - t0) * nk;
    const int ck = tid & (PD_KC - 1), cr = tid / PD_KC;
    constexpr int PD_ROWS = PD_T * PD_KC / PD_THREADS;
    constexpr int STEP = PD_THREADS / PD_KC;

    double ra[PD_ROWS], rb[VIEWS][PD_ROWS];
    auto fetch = [&](int it) {
        const int r0 = (t0 + it / nk) * PD_T;
        const int k = (it % nk) * PD_KC + ck;
        const bool kin = k < p.d;
#pragma unroll
        for (int j = 0; j < PD_ROWS; ++j) {
            const int r = r0 + cr + STEP * j, c = c0 + cr + STEP * j;
            ra[j] = (kin && r < p.na) ? pd_load(p.a, p.a64, (int64_t)r * p.lda + k) : 0.0;
            rb[0][j] = (kin && c < p.nb) ? pd_load(p.b, p.b64, (int64_t)c * p.ldb + k) : 0.0;
            if (VIEWS == 2) rb[VIEWS - 1][j] = (kin && c < p.nb) ? pd_load(p.b2, p.b264, (int64_t)c * p.ldb2 + k) : 0.0;
        }
    };

    const int col = c0 + w * 16 + lc;                            // this lane's query
    const bool cin = col < p.nb;
    const double nb0 = cin ? p.norm_b[col] : 0.0;
    const double nb1 = (VIEWS == 2 && cin) ? p.norm_b2[col] : 0.0;
    double bv[NN_L];
    int bi[NN_L];
#pragma unroll
    for (int i = 0; i < NN_L; ++i) {
        bv[i] = INFINITY;
        bi[i] = NN_NONE;
    }
    double4_t acc[VIEWS][4];
#pragma unroll
    for (int v = 0; v < VIEWS; ++v)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[v][t] = double4_t{0.0, 0.0, 0.0, 0.0};

    if (nit > 0) fetch(0);
    for (int it = 0; it < nit; ++it) {
        __syncthreads();                                         // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < PD_ROWS; ++j) {
            As[ck * PD_LD + cr + STEP * j] = ra[j];
#pragma unroll
            for (int v = 0; v < VIEWS; ++v) Bs[v][ck * PD_LD + cr + STEP * j] = rb[v][j];
        }
        __syncthreads();
        if (it + 1 < nit) fetch(it + 1);
#pragma unroll
        for (int s = 0; s < PD_KC / 4; ++s) {
            const int kk = 4 * s + lk;
            double b[VIEWS];
#pragma unroll
            for (int v = 0; v < VIEWS; ++v) b[v] = Bs[v][kk * PD_LD + w * 16 + lc];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double a = As[kk * PD_LD + 16 * t + lc];   // staged once, used by every view
#pragma unroll
                for (int v = 0; v < VIEWS; ++v) acc[v][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[v], acc[v][t], 0, 0, 0);
            }
        }
        if ((it + 1) % nk == 0) {                                // the tile's d is complete
            const int r0 = (t0 + it / nk) * PD_T;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = r0 + 16 * t + lk + 4 * e;
                    if (cin && r < p.na) {
                        const double na = p.norm_a[r];
                        double d2 = (na + nb0) - 2.0 * acc[0][t][e];
                        d2 = d2 < 0.0 ? 0.0 : d2;                // a NaN stays a NaN
                        if (VIEWS == 2) {
                            double e2 = (na + nb1) - 2.0 * acc[VIEWS - 1][t][e];
                            e2 = e2 < 0.0 ? 0.0 : e2;
                            d2 = fmin(d2, e2);                   // a NaN view is passed over
                        }
                        nn_insert(bv, bi, d2, r);
                    }
                }
#pragma unroll
                for (int v = 0; v < VIEWS; ++v) acc[v][t] = double4_t{0.0, 0.0, 0.0, 0.0};
            }
        }
    }

    // the four lanes of a query: lanes lc, lc + 16, lc + 32, lc + 48 of the wave hold disjoint rows
    for (int o = 16; o <= 32; o <<= 1) {
        double ov[NN_L];
        int oi[NN_L];
#pragma unroll
        for (int i = 0; i < NN_L; ++i) {
            ov[i] = __shfl_xor(bv[i], o);
            oi[i] = __shfl_xor(bi[i], o);
        }
#pragma unroll
        for (int i = 0; i < NN_L; ++i) nn_insert(bv, bi, ov[i], oi[i]);
    }
    if (lk == 0 && cin) {
        const int64_t at = ((int64_t)blockIdx.y * p.nb + col) * NN_L;
#pragma unroll
        for (int i = 0; i < NN_L; ++i) {
            p.part_d2[at + i] = bv[i];
            p.part_row[at + i] = bi[i];
        }
    }
}

// One thread per query: the caller's earlier lists (merge), then the splits in index order; the first k of the merged list are written.
__global__ __launch_bounds__(PD_THREADS) void nn_merge_kernel(const double* __restrict__ part_d2, const int* __restrict__ part_row, int splits,
                                                                int nb, int k, int64_t index_base, int merge, double* dist2_io,
                                                                int64_t* index_io) {
    const int c = blockIdx.x * PD_THREADS + threadIdx.x;
    if (c >= nb) return;
    constexpr int64_t NONE = INT64_MAX;
    double bv[NN_L];
    int64_t bi[NN_L];
#pragma unroll
    for (int i = 0; i < NN_L; ++i) {
        bv[i] = INFINITY;
        bi[i] = NONE;
    }
    if (merge) {
        for (int i = 0; i < k; ++i) {
            const int64_t j = index_io[(int64_t)c * k + i];
            if (j >= 0) nn_insert(bv, bi, dist2_io[(int64_t)c * k + i], j);
        }
    }
    for (int s = 0; s < splits; ++s) {
        const int64_t at = ((int64_t)s * nb + c) * NN_L;
#pragma unroll
        for (int i = 0; i < NN_L; ++i) {
            const int r = part_row[at + i];
            if (r != NN_NONE) nn_insert(bv, bi, part_d2[at + i], index_base + r);
        }
    }
#pragma unroll
    for (int i = 0; i < NN_L; ++i) {
        if (i < k) {
            const bool none = bi[i] == NONE;
            dist2_io[(int64_t)c * k + i] = none ? (double)INFINITY : bv[i];
            index_io[(int64_t)c * k + i] = none ? -1 : bi[i];
        }
    }
}

// The mirrored view, to_tensor(flipper(to_pil(img))) (:81-83, :95): x.mul(255).byte() (fp32 product, truncated; clamped to 0..255),
// mirrored along W, / 255 in fp32
__global__ __launch_bounds__(256) void hflip_u8_kernel(const float* __restrict__ in, float* __restrict__ out, int W, int64_t n) {
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % W);
        const float v = in[i - x + (W - 1 - x)] * 255.0f;
        out[i] = (float)(uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f) / 255.0f;
    }
}

// One output slot (query q, rank j) per blockIdx.x, its image split over blockIdx.y: from the piece when the slot's row lies in it, else
// from the held slot of the same query that has the row, zeros for -1 (or a row that is in neither: nothing to copy from)
__global__ __launch_bounds__(256) void nn_collect_kernel(const float* __restrict__ held, const int64_t* __restrict__ held_index,
                                                           const int64_t* __restrict__ new_index, const float* __restrict__ piece, int64_t n,
                                                           int64_t index_base, int k, int64_t chw, float* __restrict__ out) {
    const int64_t slot = blockIdx.x;
    const int64_t row = new_index[slot];
    const float* src = nullptr;
    if (row >= index_base && row - index_base < n) {
        src = piece + (row - index_base) * chw;
    } else if (row >= 0 && held_index) {
        const int64_t q0 = slot / k * k;
        for (int j = 0; j < k; ++j)
            if (held_index[q0 + j] == row) {
                src = held + (q0 + j) * chw;
                break;
            }
    }
    float* dst = out + slot * chw;
    for (int64_t i = blockIdx.y * 256L + threadIdx.x; i < chw; i += (int64_t)gridDim.y * 256) dst[i] = src ? src[i] : 0.0f;
}

}  // namespace

int64_t knn_search_scratch_bytes(int nq, int nr) {
    const PdPlan pl = pd_plan(nr, nq);
    return (2 * (int64_t)nq + nr) * sizeof(double) + (int64_t)pl.splits * nq * NN_L * (int64_t)(sizeof(double) + sizeof(int));
}

int launch_knn_search(const void* q, int q64, int64_t ldq, const void* q2, int q264, int64_t ldq2, int nq, const void* r, int r64, int64_t ldr,
                      int nr, int d, int k, int64_t index_base, int merge, double* dist2_io, int64_t* index_io, void* scratch, hipStream_t s) {
    MCVD_REQUIRE(q && r && dist2_io && index_io && scratch, "knn_search: NULL argument");
    MCVD_REQUIRE(k >= 1 && k <= NN_L, "knn_search: k = %d is outside 1..%d", k, NN_L);
    MCVD_REQUIRE(nq >= 1 && nq < (1 << 24) && nr >= 1 && nr < (1 << 24), "knn_search: %d query and %d ref rows (1 to 2^24 - 1 each)", nq, nr);
    MCVD_REQUIRE(d >= 1 && d <= 2048 && ldq >= d && ldr >= d && (!q2 || ldq2 >= d), "knn_search: bad d = %d (1 to 2048) or leading dimension", d);
    const PdPlan pl = pd_plan(nr, nq);
    double* norm_q = static_cast<double*>(scratch);
    double* norm_q2 = norm_q + nq;
    double* norm_r = norm_q2 + nq;
    if (int rc = pd_norms(q, q64, ldq, nq, d, norm_q, s)) return rc;
    if (q2)
        if (int rc = pd_norms(q2, q264, ldq2, nq, d, norm_q2, s)) return rc;
    if (int rc = pd_norms(r, r64, ldr, nr, d, norm_r, s)) return rc;
    NnArgs p;
    p.a = r;
    p.b = q;
    p.b2 = q2;
    p.a64 = r64;
    p.b64 = q64;
    p.b264 = q264;
    p.lda = ldr;
    p.ldb = ldq;
    p.ldb2 = ldq2;
    p.na = nr;
    p.nb = nq;
    p.d = d;
    p.tiles_per_split = pl.tiles_per_split;
    p.norm_a = norm_r;
    p.norm_b = norm_q;
    p.norm_b2 = norm_q2;
    p.part_d2 = norm_r + nr;
    p.part_row = reinterpret_cast<int*>(p.part_d2 + (int64_t)pl.splits * nq * NN_L);
    if (q2)
        hipLaunchKernelGGL(nn_sweep_kernel<2>, dim3(pl.colblocks, pl.splits), dim3(PD_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(nn_sweep_kernel<1>, dim3(pl.colblocks, pl.splits), dim3(PD_THREADS), 0, s, p);
    MCVD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nn_merge_kernel, dim3((nq + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, s, p.part_d2, p.part_row, pl.splits, nq, k,
                       index_base, merge, dist2_io, index_io);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_hflip_u8(const float* in, float* out, int64_t rows, int W, hipStream_t s) {
    MCVD_REQUIRE(in && out && rows > 0 && W > 0, "hflip_u8: bad arguments");
    const int64_t n = rows * W;
    const int grid = (int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
    hipLaunchKernelGGL(hflip_u8_kernel, dim3(grid), dim3(256), 0, s, in, out, W, n);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_nn_collect(const float* held, const int64_t* held_index, const int64_t* new_index, const float* piece, int64_t n, int64_t index_base,
                      int64_t slots, int k, int64_t chw, float* out, hipStream_t s) {
    MCVD_REQUIRE(new_index && piece && out && slots > 0 && slots < (1LL << 31) && k >= 1 && chw > 0 && n > 0, "nn_collect: bad arguments");
    const int64_t per = (chw + 1023) / 1024;
    hipLaunchKernelGGL(nn_collect_kernel, dim3((unsigned)slots, (unsigned)(per > 64 ? 64 : per)), dim3(256), 0, s, held, held_index, new_index, piece,
                       n, index_base, k, chw, out);
    MCVD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mcvd
