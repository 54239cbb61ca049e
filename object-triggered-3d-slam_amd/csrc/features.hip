// features.hip — pipelines.registration.compute_fpfh_feature and correspondences_from_features on MI355X
// ("features").
//
// FPFH, three kernels over the neighbour lists of nb_list.h (the lists of normals.hip, up to 128 entries here):
//   k_feat_lists : one lane per query in the grid's sorted cell order: the search, then the list (length, indices, d2)
//                  to the FEAT_LISTS workspace, entry-major ([t][point]) so the two readers below, one lane per point
//                  in input order, load coalesced.
//   k_spfh       : one lane per point: the pair features of entries 1 .. len-1 in list order, binned into the lane's
//                  33-bin histogram in LDS (bin b of lane l at [b * 64 + l]: conflict-free).
//   k_fpfh       : one lane per point: the neighbours' SPFH rows (264 contiguous bytes each) weighted by 1 / d2, the
//                  three block sums in (neighbour outer, component inner) order, the 33 accumulators in registers.
// Matching, an exhaustive sweep:
//   k_match      : one lane per query row, held in registers (padded with zeros to the instantiation's width, which
//                  adds exact zeros to the sequential sum); the targets pass through LDS in tiles and every lane reads
//                  the same address (broadcast).  Ascending target index and a strict < give the (d2, index) minimum.
//                  The target range is split over gridDim.y so that a small n still fills the device.
//   k_match_merge: the (d2, index) minimum over the splits (order independent, so deterministic).
//   the mutual filter is k_match with the roles swapped and a stable compaction (compact.h) of the pairs that agree.
// Everything is float64 without contraction, no floating-point atomics; acos and atan2 (device library) are the only
// operations whose last bits may differ from a host restatement, and they only decide a swap and a bin.
#include <algorithm>
#include <cmath>

#include "compact.h"
#include "nb_list.h"
#include "sor.h"

namespace ot {

constexpr int FEAT_BINS = 33;
constexpr int MATCH_SMALL = 33, MATCH_SMALL_TILE = 64;  // dim <= 33: 64 targets x 33 doubles = 16.5 KiB per tile
constexpr int MATCH_LARGE = 128, MATCH_LARGE_TILE = 32;  // dim <= 128: 32 targets x 128 doubles = 32 KiB per tile
constexpr int MATCH_WORKGROUPS = 2048;  // workgroups a sweep aims for (8 per CU): decides the split, never a result

// r2 <= 0: KNN; r2 > 0: hybrid.  len[n], idx / d2: [min(k, n)][n]
template <int KMAX>
__global__ __launch_bounds__(64) void k_feat_lists(GridDev g, int64_t n, int k, double r2, int* __restrict__ len,
                                                   unsigned* __restrict__ idx, double* __restrict__ d2) {
    __shared__ double s_d[KMAX * 64];
    __shared__ unsigned s_i[KMAX * 64];
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    double* Ld = s_d + threadIdx.x;
    unsigned* Li = s_i + threadIdx.x;
    const int kk = (int)((int64_t)k < n ? k : n);  // <= KMAX (host)
    const int m = nb_search(g, n, j, kk, r2, Ld, Li);
    const int64_t i = g.sidx[j];
    len[i] = m;
    for (int t = 0; t < m; ++t) {
        idx[(int64_t)t * n + i] = Li[t * 64];
        d2[(int64_t)t * n + i] = Ld[t * 64];
    }
}

struct Vec3 {
    double x, y, z;
};
__device__ inline Vec3 vcross(Vec3 a, Vec3 b) {
    return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ inline double vdot(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline Vec3 vload(const double* __restrict__ p, int64_t i) { return Vec3{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]}; }

// Open3D's ComputePairFeatures: f[0..2] = (f1, f2, f3) of DESIGN.md §4 "features"
__device__ inline void pair_features(Vec3 p1, Vec3 n1, Vec3 p2, Vec3 n2, double f[3]) {
    f[0] = 0.0, f[1] = 0.0, f[2] = 0.0;
    Vec3 dp{p2.x - p1.x, p2.y - p1.y, p2.z - p1.z};
    const double dist = sqrt(vdot(dp, dp));
    if (dist == 0.0) return;
    const double a1 = vdot(n1, dp) / dist, a2 = vdot(n2, dp) / dist;
    double f3;
    if (acos(fabs(a1)) > acos(fabs(a2))) {
        const Vec3 t = n1;
        n1 = n2;
        n2 = t;
        dp = Vec3{-dp.x, -dp.y, -dp.z};
        f3 = -a2;
    } else {
        f3 = a1;
    }
    Vec3 v = vcross(dp, n1);
    const double vn = sqrt(vdot(v, v));
    if (vn == 0.0) return;
    v = Vec3{v.x / vn, v.y / vn, v.z / vn};
    const Vec3 w = vcross(n1, v);
    f[1] = vdot(v, n2);
    f[0] = atan2(vdot(w, n2), vdot(n1, n2));
    f[2] = f3;
}

// floor of the bin coordinate, clamped to 0 .. 10 (a NaN lands in bin 0)
__device__ inline int feat_bin(double c) {
    double h = floor(c);
    if (!(h >= 0.0)) h = 0.0;
    if (h > 10.0) h = 10.0;
    return (int)h;
}

__global__ __launch_bounds__(64) void k_spfh(const double* __restrict__ xyz, const double* __restrict__ nrm, int64_t n,
                                             const int* __restrict__ len, const unsigned* __restrict__ idx,
                                             double* __restrict__ spfh) {
    __shared__ double s_h[FEAT_BINS * 64];
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double* H = s_h + threadIdx.x;
    for (int b = 0; b < FEAT_BINS; ++b) H[b * 64] = 0.0;
    const int m = len[i];
    if (m > 1) {
        const double inc = 100.0 / (double)(m - 1);
        const Vec3 p1 = vload(xyz, i), n1 = vload(nrm, i);
        for (int t = 1; t < m; ++t) {
            const int64_t q = idx[(int64_t)t * n + i];
            double f[3];
            pair_features(p1, n1, vload(xyz, q), vload(nrm, q), f);
            const int h1 = feat_bin(11 * (f[0] + M_PI) / (2.0 * M_PI));
            const int h2 = feat_bin(11 * (f[1] + 1.0) * 0.5);
            const int h3 = feat_bin(11 * (f[2] + 1.0) * 0.5);
            H[h1 * 64] += inc;
            H[(11 + h2) * 64] += inc;
            H[(22 + h3) * 64] += inc;
        }
    }
    double* out = spfh + i * FEAT_BINS;
    for (int b = 0; b < FEAT_BINS; ++b) out[b] = H[b * 64];
}

__global__ __launch_bounds__(64) void k_fpfh(const double* __restrict__ spfh, int64_t n, const int* __restrict__ len,
                                             const unsigned* __restrict__ idx, const double* __restrict__ d2,
                                             double* __restrict__ fpfh) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double F[FEAT_BINS];
#pragma unroll
    for (int j = 0; j < FEAT_BINS; ++j) F[j] = 0.0;
    const int m = len[i];
    if (m > 1) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (int t = 1; t < m; ++t) {
            const double d = d2[(int64_t)t * n + i];
            if (d == 0.0) continue;
            const double* row = spfh + (int64_t)idx[(int64_t)t * n + i] * FEAT_BINS;
#pragma unroll
            for (int j = 0; j < FEAT_BINS; ++j) {
                const double val = row[j] / d;
                sum[j / 11] += val;
                F[j] += val;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (sum[c] != 0.0) sum[c] = 100.0 / sum[c];
        const double* own = spfh + i * FEAT_BINS;
#pragma unroll
        for (int j = 0; j < FEAT_BINS; ++j) {
            F[j] *= sum[j / 11];
            F[j] += own[j];
        }
    }
    double* out = fpfh + i * FEAT_BINS;
#pragma unroll
    for (int j = 0; j < FEAT_BINS; ++j) out[j] = F[j];
}

// ------------------------------------------------------------------------------------------ matching
// Rows [blockIdx.x * 64, + 64) of a against rows [blockIdx.y * per_split, + per_split) of b (per_split a multiple of
// TT).  pd / pi: [gridDim.y][na] minima of the splits.
template <int DIMP, int TT>
__global__ __launch_bounds__(64) void k_match(const double* __restrict__ a, int64_t na, const double* __restrict__ b,
                                              int64_t nb, int dim, int64_t per_split, double* __restrict__ pd,
                                              int* __restrict__ pi) {
    __shared__ double s_t[TT * DIMP];
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < na;
    double s[DIMP];
#pragma unroll
    for (int j = 0; j < DIMP; ++j) s[j] = (live && j < dim) ? a[i * dim + j] : 0.0;
    const int64_t t0 = (int64_t)blockIdx.y * per_split;
    const int64_t t1 = t0 + per_split < nb ? t0 + per_split : nb;
    double best = INFINITY;
    int64_t bi = t0;
    for (int64_t base = t0; base < t1; base += TT) {
        const int cnt = (int)(t1 - base < TT ? t1 - base : TT);
        __syncthreads();  // the previous tile was read by every lane
        for (int e = threadIdx.x; e < cnt * DIMP; e += 64) {
            const int r = e / DIMP, j = e - r * DIMP;
            s_t[e] = j < dim ? b[(base + r) * dim + j] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
            const double* t = s_t + r * DIMP;
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < DIMP; ++j) {
                const double df = s[j] - t[j];
                d += df * df;
            }
            if (d < best) {
                best = d;
                bi = base + r;
            }
        }
    }
    if (live) {
        pd[(int64_t)blockIdx.y * na + i] = best;
        pi[(int64_t)blockIdx.y * na + i] = (int)bi;
    }
}

__global__ __launch_bounds__(256) void k_match_merge(const double* __restrict__ pd, const int* __restrict__ pi,
                                                     int64_t na, int splits, int* __restrict__ match) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    double best = pd[i];
    int bi = pi[i];
    for (int s = 1; s < splits; ++s) {
        const double d = pd[(int64_t)s * na + i];
        const int id = pi[(int64_t)s * na + i];
        if (d < best || (d == best && id < bi)) {
            best = d;
            bi = id;
        }
    }
    match[i] = bi;
}

__global__ __launch_bounds__(256) void k_match_pairs(const int* __restrict__ match, int64_t n, int32_t* __restrict__ corr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    corr[i * 2] = (int32_t)i;
    corr[i * 2 + 1] = match[i];
}

struct MutualPred {
    const int* ms;
    const int* mt;
    __device__ bool operator()(int64_t i) const { return mt[ms[i]] == (int)i; }
};
struct MutualEmit {
    const int* ms;
    int32_t* corr;
    __device__ void operator()(int64_t i, int64_t pos) const {
        corr[pos * 2] = (int32_t)i;
        corr[pos * 2 + 1] = ms[i];
    }
};

static int match_tile(int dim) { return dim <= MATCH_SMALL ? MATCH_SMALL_TILE : MATCH_LARGE_TILE; }

// how the nb targets are split for na queries: {splits, targets per split (a multiple of the tile)}
static void match_split(int64_t na, int64_t nb, int dim, int& splits, int64_t& per_split) {
    const int64_t TT = match_tile(dim);
    const int64_t blocks = (na + 63) / 64, tiles = (nb + TT - 1) / TT;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, MATCH_WORKGROUPS / blocks));
    per_split = (tiles + want - 1) / want * TT;
    splits = (int)((nb + per_split - 1) / per_split);
}

// match[i] = the row of b nearest to row i of a by (d2, index); pd / pi hold the splits' minima.  Only queued.
static ot_status match_rows(const double* a, int64_t na, const double* b, int64_t nb, int dim, double* pd, int* pi,
                            int* match, hipStream_t stream) {
    int splits;
    int64_t per_split;
    match_split(na, nb, dim, splits, per_split);
    const dim3 grid((unsigned)((na + 63) / 64), (unsigned)splits), block(64);
    if (dim <= MATCH_SMALL)
        hipLaunchKernelGGL((k_match<MATCH_SMALL, MATCH_SMALL_TILE>), grid, block, 0, stream, a, na, b, nb, dim,
                           per_split, pd, pi);
    else
        hipLaunchKernelGGL((k_match<MATCH_LARGE, MATCH_LARGE_TILE>), grid, block, 0, stream, a, na, b, nb, dim,
                           per_split, pd, pi);
    hipLaunchKernelGGL(k_match_merge, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream, (const double*)pd,
                       (const int*)pi, na, splits, match);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_compute_fpfh_feature(const double* xyz, const double* normals, int64_t n, int32_t knn, double radius,
                                  double* fpfh_out, double* spfh_out, void* stream_) {
    hipStream_t stream = S(stream_);
    if (knn < 1 || knn > 128)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ComputeFPFHFeature] knn / max_nn must lie in 1..128 (the neighbour "
                                             "list is kept on chip), got " + std::to_string(knn));
    if (std::isnan(radius)) return fail(OT_ERR_INVALID_ARGUMENT, "[ComputeFPFHFeature] radius is NaN");
    if (n <= 0) return OT_OK;
    if (!xyz || !normals || !fpfh_out || n > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ComputeFPFHFeature] invalid buffers");
    // cells sized as SOR's (sor.h): the grid only changes speed
    double mn[3], mx[3];
    GridBuild gb;
    ot_status st = occupancy_grid(xyz, n, sor_cell_target(knn), GRID_NBR3, mn, mx, stream, gb);
    if (st != OT_OK) return st;
    const size_t kk = (size_t)std::min<int64_t>(knn, n);
    auto [len, idx, d2] = carve(scratch_of(Slot::FEAT_LISTS), Arr<int>{(size_t)n}, Arr<unsigned>{kk * (size_t)n},
                                Arr<double>{kk * (size_t)n});
    if (!len) return fail(OT_ERR_HIP, "scratch allocation failed");
    double* spfh = spfh_out;
    if (!spfh) {
        spfh = (double*)scratch((size_t)n * FEAT_BINS * sizeof(double), Slot::FEAT_SPFH);
        if (!spfh) return fail(OT_ERR_HIP, "scratch allocation failed");
    }
    const double r2 = radius > 0.0 ? radius * radius : 0.0;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (knn <= 32) hipLaunchKernelGGL(k_feat_lists<32>, grid, block, 0, stream, gb.g, n, (int)knn, r2, len, idx, d2);
    else if (knn <= 64) hipLaunchKernelGGL(k_feat_lists<64>, grid, block, 0, stream, gb.g, n, (int)knn, r2, len, idx, d2);
    else hipLaunchKernelGGL(k_feat_lists<128>, grid, block, 0, stream, gb.g, n, (int)knn, r2, len, idx, d2);
    hipLaunchKernelGGL(k_spfh, grid, block, 0, stream, xyz, normals, n, (const int*)len, (const unsigned*)idx, spfh);
    hipLaunchKernelGGL(k_fpfh, grid, block, 0, stream, (const double*)spfh, n, (const int*)len, (const unsigned*)idx,
                       (const double*)d2, fpfh_out);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_correspondences_from_features(const double* src, int64_t n, const double* tgt, int64_t m, int32_t dim,
                                           int32_t mutual_filter, double mutual_consistency_ratio, int32_t* corr_out,
                                           int64_t* n_corr_host, int32_t* fell_back_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (dim < 1 || dim > MATCH_LARGE)
        return fail(OT_ERR_INVALID_ARGUMENT, "[CorrespondencesFromFeatures] the feature dimension must lie in 1..128, "
                                             "got " + std::to_string(dim));
    if (!n_corr_host) return fail(OT_ERR_INVALID_ARGUMENT, "[CorrespondencesFromFeatures] n_corr_host is NULL");
    *n_corr_host = 0;
    if (fell_back_host) *fell_back_host = 0;
    if (n <= 0) return OT_OK;
    if (m <= 0) return fail(OT_ERR_INVALID_ARGUMENT, "[CorrespondencesFromFeatures] the target has no features");
    if (!src || !tgt || !corr_out || n > 0x7FFFFFFF || m > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, "[CorrespondencesFromFeatures] invalid buffers");
    int ss, st_;
    int64_t per;
    match_split(n, m, dim, ss, per);
    match_split(m, n, dim, st_, per);
    const size_t parts = std::max((size_t)ss * (size_t)n, mutual_filter ? (size_t)st_ * (size_t)m : (size_t)0);
    auto [pd, pi, ms, mt] = carve(scratch_of(Slot::FEAT_MATCH), Arr<double>{parts}, Arr<int>{parts},
                                  Arr<int>{(size_t)n}, Arr<int>{mutual_filter ? (size_t)m : (size_t)0});
    if (!pd) return fail(OT_ERR_HIP, "scratch allocation failed");
    ot_status st = match_rows(src, n, tgt, m, dim, pd, pi, ms, stream);
    if (st != OT_OK) return st;
    if (mutual_filter) {
        st = match_rows(tgt, m, src, n, dim, pd, pi, mt, stream);  // in stream order after the merge of the first
        if (st != OT_OK) return st;
        int64_t kept = 0;
        st = compact(n, MutualPred{ms, mt}, MutualEmit{ms, corr_out}, stream, &kept, Slot::FEAT_COMPACT);
        if (st != OT_OK) return st;
        if ((double)kept >= mutual_consistency_ratio * (double)n) {
            *n_corr_host = kept;
            return OT_OK;
        }
        if (fell_back_host) *fell_back_host = 1;
    }
    hipLaunchKernelGGL(k_match_pairs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const int*)ms, n,
                       corr_out);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n_corr_host = n;
    return OT_OK;
}

}  // extern "C"
