// segment_plane.hip — PointCloud::SegmentPlane (seeded RANSAC plane fit) on MI355X; the definition built against is
// DESIGN.md §4, "Plane segmentation" (restated in numpy by tests/segment_plane_ref.py).
//
// The serial loop's control flow depends on the candidates' inlier COUNTS alone (the break threshold is a function of
// the best fitness, and an equal-fitness replacement recomputes the same threshold), so the loop is replayed on the
// host from integer counts, a chunk of iterations at a time:
//   k_sp_candidates : one lane per iteration.  Draws the sample from the counter RNG (rng.h), fits its plane
//                     (ComputeTrianglePlane, or GetPlaneFromPoints over the sample run serially in the lane) and
//                     starts the candidate's counter (top bit set: a zero plane, which is skipped without counting).
//   k_sp_count      : the sweep.  A workgroup keeps 1024 points in registers (4 per lane) and walks SP_CPB candidates
//                     whose coefficients arrive through uniform loads; per candidate the inliers of a wave are the
//                     popcounts of 4 ballots, the 4 waves meet in LDS, and one integer atomic per candidate and
//                     workgroup reaches global memory.  Integer sums: the same bits whatever the order.
//   k_sp_mail       : the chunk's counts and planes to pinned host memory, then the sequence word (mail_wait).
// The host replays the loop on the counts (break threshold with the host's libm: a device log / pow one ulp off could
// change trunc() and with it which iterations run) and stops queueing chunks once the loop has broken.
// If several evaluated candidates hold the best count k*, inlier_rmse decides: err of those candidates alone is the
// serial sum over all points of (inlier ? dist : +0.0) -- adding +0.0 to a non-negative partial sum is exact -- formed
// by the exact chains of chain.h.  The final pass compacts the best plane's inliers stably (compact.h), gathers their
// coordinates and takes the centroid and moment sums through the same chains; the 3x3 determinant step runs on the
// host.  No floating-point atomics anywhere.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "chain.h"
#include "compact.h"
#include "rng.h"
#include "tsdf.h"  // mail_wait

namespace ot {

constexpr int SP_MAX_RANSAC_N = 32;  // the sample lives in one lane's private memory
constexpr int SP_CHUNK = 256;        // iterations per round trip (measured: DESIGN.md §4.1); the default 100 is one chunk
constexpr int SP_CHUNK_MAX = 1024;
constexpr int SP_THREADS = 256, SP_PTS = 4, SP_TILE = SP_THREADS * SP_PTS;
constexpr int SP_CPB = 64;        // candidates a workgroup walks (grid.y covers the chunk)
constexpr int SP_TIE_JOBS = 16;   // masked distance arrays summed side by side in the rmse tie-break
constexpr unsigned SP_ZERO = 0x80000000u;  // counter bit: the candidate is the zero plane
// a lane gives up after this many draws (N >= ransac_n distinct indices exist, so a draw is new with probability
// >= 1 / N; for the worst case N = 3 the chance of getting here is (2/3)^65536): the candidate is then a zero plane
constexpr unsigned long long SP_DRAW_CAP = 1ull << 16;

struct Plane4 {
    double v[4];
};
struct PlaneSet {
    Plane4 p[SP_TIE_JOBS];
};

// GetPlaneFromPoints' last step: the plane through centroid c whose normal is the best-conditioned of the three
// cofactor solutions of the moment matrix
__host__ __device__ inline void plane_from_moments(const double c[3], double xx, double xy, double xz, double yy,
                                                   double yz, double zz, double out[4]) {
    const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
    double a, b, g;
    if (det_x > det_y && det_x > det_z) {
        a = det_x, b = xz * yz - xy * zz, g = xy * yz - xz * yy;
    } else if (det_y > det_z) {
        a = xz * yz - xy * zz, b = det_y, g = xy * xz - yz * xx;
    } else {
        a = xy * yz - xz * yy, b = xy * xz - yz * xx, g = det_z;
    }
    const double norm = sqrt((a * a + b * b) + g * g);
    if (norm == 0.0) {
        out[0] = out[1] = out[2] = out[3] = 0.0;
        return;
    }
    a /= norm, b /= norm, g /= norm;
    out[0] = a, out[1] = b, out[2] = g;
    out[3] = -((a * c[0] + b * c[1]) + g * c[2]);
}

__device__ inline bool sp_inlier(const double* __restrict__ xyz, int64_t i, const double pl[4], double thr,
                                 double& dist) {
    dist = fabs(((pl[0] * xyz[i * 3] + pl[1] * xyz[i * 3 + 1]) + pl[2] * xyz[i * 3 + 2]) + pl[3]);
    return dist < thr;
}

__global__ __launch_bounds__(64) void k_sp_candidates(const double* __restrict__ xyz, int64_t n, int ransac_n,
                                                      unsigned long long seed, long long it0, int ncand,
                                                      double* __restrict__ planes, unsigned* __restrict__ counts) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ncand) return;
    const unsigned long long it = (unsigned long long)(it0 + c);
    int idx[SP_MAX_RANSAC_N];
    int kept = 0;
    for (unsigned long long t = 0; kept < ransac_n && t < SP_DRAW_CAP; ++t) {
        const int i = (int)(rng_word(seed, (it << 32) + t) % (unsigned long long)n);
        bool dup = false;
        for (int j = 0; j < kept; ++j) dup |= idx[j] == i;
        if (!dup) idx[kept++] = i;
    }
    double pl[4] = {0.0, 0.0, 0.0, 0.0};
    if (kept == ransac_n) {
        if (ransac_n == 3) {  // ComputeTrianglePlane
            const double* p0 = xyz + (int64_t)idx[0] * 3;
            const double* p1 = xyz + (int64_t)idx[1] * 3;
            const double* p2 = xyz + (int64_t)idx[2] * 3;
            const double e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
            const double e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
            double a = e0[1] * e1[2] - e0[2] * e1[1], b = e0[2] * e1[0] - e0[0] * e1[2],
                   g = e0[0] * e1[1] - e0[1] * e1[0];
            const double norm = sqrt((a * a + b * b) + g * g);
            if (norm != 0.0) {
                a /= norm, b /= norm, g /= norm;
                pl[0] = a, pl[1] = b, pl[2] = g;
                pl[3] = -((a * p0[0] + b * p0[1]) + g * p0[2]);
            }
        } else {  // GetPlaneFromPoints over the sample, in draw order
            double s[3] = {0.0, 0.0, 0.0};
            for (int j = 0; j < ransac_n; ++j)
                for (int a = 0; a < 3; ++a) s[a] += xyz[(int64_t)idx[j] * 3 + a];
            const double k = (double)ransac_n;
            const double ctr[3] = {s[0] / k, s[1] / k, s[2] / k};
            double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
            for (int j = 0; j < ransac_n; ++j) {
                const double* p = xyz + (int64_t)idx[j] * 3;
                const double rx = p[0] - ctr[0], ry = p[1] - ctr[1], rz = p[2] - ctr[2];
                xx += rx * rx, xy += rx * ry, xz += rx * rz;
                yy += ry * ry, yz += ry * rz, zz += rz * rz;
            }
            plane_from_moments(ctr, xx, xy, xz, yy, yz, zz, pl);
        }
    }
    const bool zero = pl[0] == 0.0 && pl[1] == 0.0 && pl[2] == 0.0 && pl[3] == 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) planes[(int64_t)c * 4 + a] = pl[a];
    counts[c] = zero ? SP_ZERO : 0u;
}

// grid: (point tiles, ceil(ncand / SP_CPB))
__global__ __launch_bounds__(SP_THREADS) void k_sp_count(const double* __restrict__ xyz, int64_t n,
                                                         const double* __restrict__ planes, int ncand, double thr,
                                                         unsigned* __restrict__ counts) {
    __shared__ unsigned wc[SP_THREADS / 64][SP_CPB];
    const int64_t tile = (int64_t)blockIdx.x * SP_TILE;
    const int c0 = blockIdx.y * SP_CPB;
    const int nc = min(SP_CPB, ncand - c0);
    double x[SP_PTS], y[SP_PTS], z[SP_PTS];
    bool live[SP_PTS];
#pragma unroll
    for (int k = 0; k < SP_PTS; ++k) {
        const int64_t i = tile + (int64_t)k * SP_THREADS + threadIdx.x;
        live[k] = i < n;
        x[k] = live[k] ? xyz[i * 3] : 0.0;
        y[k] = live[k] ? xyz[i * 3 + 1] : 0.0;
        z[k] = live[k] ? xyz[i * 3 + 2] : 0.0;
    }
    const int wave = threadIdx.x >> 6;
    const bool first = lane_id() == 0;
    for (int c = 0; c < nc; ++c) {
        const double* pl = planes + (int64_t)(c0 + c) * 4;  // the same address in every lane
        const double a = pl[0], b = pl[1], g = pl[2], d = pl[3];
        unsigned cnt = 0;
        if (!(a == 0.0 && b == 0.0 && g == 0.0 && d == 0.0)) {
#pragma unroll
            for (int k = 0; k < SP_PTS; ++k) {
                const bool in = live[k] && fabs(((a * x[k] + b * y[k]) + g * z[k]) + d) < thr;
                cnt += (unsigned)__popcll(__ballot(in));
            }
        }
        if (first) wc[wave][c] = cnt;
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < SP_THREADS / 64; ++w) t += wc[w][threadIdx.x];
        if (t) atomicAdd(&counts[c0 + threadIdx.x], t);
    }
}

// mail (pinned, coherent): cap count words, cap planes (8 words each), the sequence word
__global__ __launch_bounds__(256) void k_sp_mail(const double* __restrict__ planes, const unsigned* __restrict__ counts,
                                                 int ncand, int cap, unsigned* mail, unsigned seq) {
    const unsigned* pw = (const unsigned*)planes;
    for (int e = threadIdx.x; e < ncand; e += 256) mail[e] = counts[e];
    for (int e = threadIdx.x; e < ncand * 8; e += 256) mail[cap + e] = pw[e];
    __threadfence_system();  // the values reach the host before the sequence word
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(mail + cap * 9, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the tie-break's inputs: out[j][i] = dist_i against plane j for its inliers, +0.0 for the rest.  grid: (n / 256, jobs)
__global__ __launch_bounds__(256) void k_sp_masked(const double* __restrict__ xyz, int64_t n, PlaneSet ps, double thr,
                                                   double* __restrict__ out, int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double dist;
    const bool in = sp_inlier(xyz, i, ps.p[blockIdx.y].v, thr, dist);
    out[(int64_t)blockIdx.y * stride + i] = in ? dist : 0.0;
}

struct SpPred {
    const double* xyz;
    Plane4 pl;
    double thr;
    __device__ bool operator()(int64_t i) const {
        double dist;
        return sp_inlier(xyz, i, pl.v, thr, dist);
    }
};
// the inlier's index and its coordinates, one array per axis (the chains' inputs)
struct SpEmit {
    const double* xyz;
    int64_t* idx;
    double* g;
    int64_t stride;
    __device__ void operator()(int64_t i, int64_t pos) const {
        idx[pos] = i;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a * stride + pos] = xyz[i * 3 + a];
    }
};

// the six products of r = p - centroid per inlier, one array each: xx, xy, xz, yy, yz, zz
__global__ __launch_bounds__(256) void k_sp_moments(const double* __restrict__ g, int64_t k, int64_t stride, double cx,
                                                    double cy, double cz, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const double rx = g[i] - cx, ry = g[stride + i] - cy, rz = g[2 * stride + i] - cz;
    out[i] = rx * rx;
    out[stride + i] = rx * ry;
    out[2 * stride + i] = rx * rz;
    out[3 * stride + i] = ry * ry;
    out[4 * stride + i] = ry * rz;
    out[5 * stride + i] = rz * rz;
}

// test hooks (otx_segment_plane_chunk / otx_segment_plane_profile): the chunk size, and the last call's stage times
static int g_sp_chunk = SP_CHUNK;
struct SpTimes {
    double count_ms, loop_ms, tie_ms, chain_ms, final_ms, chunks, holders, evaluated;
};
static thread_local SpTimes g_sp_times = {};
static thread_local bool g_sp_prof = false;
static thread_local unsigned g_sp_seq = 0;

// the serial loop's break threshold after a replacement (host libm)
static long long sp_break_iteration(double fitness, int ransac_n, double probability, int num_iterations) {
    if (!(fitness < 1.0)) return 0;
    const double q = std::log(1.0 - probability) / std::log(1.0 - std::pow(fitness, (double)ransac_n));
    if (!(std::isfinite(q) && q >= 0.0)) return num_iterations;
    return (long long)std::min(std::trunc(q), (double)num_iterations);
}

// out[j] = the serial sum of n values at x + j * stride, j < jobs (synchronises); ws: chain_aux_bytes(n) * jobs +
// (sizeof(ChainJob) + 8) * jobs + 128 bytes of device memory
static ot_status sp_chain_sums(const double* x, int64_t stride, int64_t n, int jobs, char* ws, double* out_host,
                               hipStream_t stream) {
    std::vector<ChainJob> jb((size_t)jobs);
    double* sums = (double*)ws;
    char* cur = (char*)(((uintptr_t)(sums + jobs) + 63) & ~(uintptr_t)63);
    for (int j = 0; j < jobs; ++j) {
        jb[j] = ChainJob{};
        jb[j].x = x + (int64_t)j * stride;
        jb[j].n = n;
        jb[j].out = sums + j;
        cur = chain_aux(cur, n, jb[j]);
    }
    ChainJob* djobs = (ChainJob*)cur;
    OT_HIP_TRY(hipMemcpyAsync(djobs, jb.data(), sizeof(ChainJob) * jobs, hipMemcpyHostToDevice, stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (g_sp_prof) {
        OT_HIP_TRY(hipEventCreate(&e0));
        OT_HIP_TRY(hipEventCreate(&e1));
        OT_HIP_TRY(hipEventRecord(e0, stream));
    }
    launch_sum_chains(djobs, jobs, n, stream);
    OT_LAUNCH_CHECK();
    if (g_sp_prof) OT_HIP_TRY(hipEventRecord(e1, stream));
    OT_HIP_TRY(hipMemcpyAsync(out_host, sums, sizeof(double) * jobs, hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (g_sp_prof) {
        float ms = 0.f;
        OT_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        g_sp_times.chain_ms += ms;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    return OT_OK;
}
static size_t sp_chain_ws_bytes(int64_t n, int jobs) {
    return (chain_aux_bytes(n) + sizeof(ChainJob) + 8) * (size_t)jobs + 256;
}

struct SpHolder {
    Plane4 pl;
    long long it;
};

static ot_status segment_plane_run(const double* xyz, int64_t n, double thr, int ransac_n, int num_iterations,
                                   double probability, unsigned long long seed, double* plane_host, int64_t* inliers,
                                   int64_t* n_inliers_host, int32_t* evaluated_host, hipStream_t stream) {
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    g_sp_times = SpTimes{};
    const int chunk = g_sp_chunk;

    // ---- the loop, replayed on counts
    long long count = 0, break_iteration = std::numeric_limits<long long>::max();
    unsigned best_k = 0;
    std::vector<SpHolder> holders;  // the evaluated candidates that hold best_k, in iteration order
    const clk::time_point t_loop = clk::now();
    if (num_iterations > 0) {
        auto [planes, counts] =
            carve(scratch_of(Slot::SP_CANDIDATES), Arr<double>{(size_t)chunk * 4}, Arr<unsigned>{(size_t)chunk});
        unsigned* mail =
            (unsigned*)pinned_scratch(sizeof(unsigned) * ((size_t)chunk * 9 + 2), PinnedSlot::SP_MAIL, true);
        if (!planes || !mail) return fail(OT_ERR_HIP, "scratch allocation failed");
        mail[chunk * 9] = 0;  // below every sequence number sent (nothing of an earlier call is in flight)
        const unsigned tiles = (unsigned)((n + SP_TILE - 1) / SP_TILE);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (g_sp_prof) {
            OT_HIP_TRY(hipEventCreate(&e0));
            OT_HIP_TRY(hipEventCreate(&e1));
        }
        bool broke = false;
        for (long long it0 = 0; it0 < num_iterations && !broke; it0 += chunk) {
            const int ncand = (int)std::min<long long>(chunk, num_iterations - it0);
            if (++g_sp_seq == 0) ++g_sp_seq;
            hipLaunchKernelGGL(k_sp_candidates, dim3((unsigned)((ncand + 63) / 64)), dim3(64), 0, stream, xyz, n,
                               ransac_n, seed, it0, ncand, planes, counts);
            if (g_sp_prof) OT_HIP_TRY(hipEventRecord(e0, stream));
            hipLaunchKernelGGL(k_sp_count, dim3(tiles, (unsigned)((ncand + SP_CPB - 1) / SP_CPB)), dim3(SP_THREADS), 0,
                               stream, xyz, n, (const double*)planes, ncand, thr, counts);
            if (g_sp_prof) OT_HIP_TRY(hipEventRecord(e1, stream));
            hipLaunchKernelGGL(k_sp_mail, dim3(1), dim3(256), 0, stream, (const double*)planes,
                               (const unsigned*)counts, ncand, chunk, mail, g_sp_seq);
            OT_LAUNCH_CHECK();
            ot_status st = mail_wait(mail + chunk * 9, g_sp_seq, stream);
            if (st != OT_OK) return st;
            if (g_sp_prof) {
                float ms = 0.f;
                OT_HIP_TRY(hipEventSynchronize(e1));
                OT_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
                g_sp_times.count_ms += ms;
            }
            g_sp_times.chunks += 1.0;
            for (int c = 0; c < ncand; ++c) {
                if (count > break_iteration) {  // stays true: nothing later is evaluated
                    broke = true;
                    break;
                }
                const unsigned k = mail[c];
                if (k & SP_ZERO) continue;  // a zero plane is skipped and does not count
                if (k > best_k || (k == best_k && k > 0)) {
                    SpHolder h;
                    std::memcpy(h.pl.v, mail + chunk + (size_t)c * 8, sizeof(h.pl.v));
                    h.it = it0 + c;
                    if (k > best_k) {
                        best_k = k;
                        holders.clear();
                        break_iteration =
                            sp_break_iteration((double)k / (double)n, ransac_n, probability, num_iterations);
                    }
                    holders.push_back(h);
                }
                ++count;
            }
        }
        if (g_sp_prof) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    }
    g_sp_times.loop_ms = ms_since(t_loop);
    g_sp_times.holders = (double)holders.size();
    g_sp_times.evaluated = (double)count;

    // ---- equal counts: the smallest inlier_rmse wins, the earliest among exactly equal ones
    Plane4 best = {{0.0, 0.0, 0.0, 0.0}};
    const clk::time_point t_tie = clk::now();
    if (holders.size() == 1) {
        best = holders[0].pl;
    } else if (holders.size() > 1) {
        const int64_t stride = (n + 1) & ~(int64_t)1;
        auto [masked, ws] = carve(scratch_of(Slot::SP_TIES), Arr<double>{(size_t)stride * SP_TIE_JOBS},
                                  Arr<char>{sp_chain_ws_bytes(n, SP_TIE_JOBS)});
        if (!masked) return fail(OT_ERR_HIP, "scratch allocation failed");
        const double root_k = std::sqrt((double)best_k);
        double best_rmse = 0.0;
        for (size_t h0 = 0; h0 < holders.size(); h0 += SP_TIE_JOBS) {
            const int jobs = (int)std::min<size_t>(SP_TIE_JOBS, holders.size() - h0);
            PlaneSet ps;
            std::memset(&ps, 0, sizeof(ps));
            for (int j = 0; j < jobs; ++j) ps.p[j] = holders[h0 + j].pl;
            hipLaunchKernelGGL(k_sp_masked, dim3((unsigned)((n + 255) / 256), (unsigned)jobs), dim3(256), 0, stream, xyz,
                               n, ps, thr, masked, stride);
            OT_LAUNCH_CHECK();
            double err[SP_TIE_JOBS];
            ot_status st = sp_chain_sums(masked, stride, n, jobs, ws, err, stream);
            if (st != OT_OK) return st;
            for (int j = 0; j < jobs; ++j) {
                const double rmse = err[j] / root_k;
                if (h0 + j == 0 || rmse < best_rmse) {
                    best_rmse = rmse;
                    best = holders[h0 + j].pl;
                }
            }
        }
    }
    g_sp_times.tie_ms = ms_since(t_tie);
    g_sp_times.chain_ms = 0.0;  // reported for the refit alone

    // ---- the best plane's inliers, ascending, and GetPlaneFromPoints over them
    const clk::time_point t_final = clk::now();
    int64_t k = 0;
    double sums[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool best_zero = best.v[0] == 0.0 && best.v[1] == 0.0 && best.v[2] == 0.0 && best.v[3] == 0.0;
    if (!best_zero) {
        const int64_t stride = (n + 1) & ~(int64_t)1;
        auto [g, prod, ws] = carve(scratch_of(Slot::SP_FINAL), Arr<double>{(size_t)stride * 3},
                                   Arr<double>{(size_t)stride * 6}, Arr<char>{sp_chain_ws_bytes(n, 6)});
        if (!g) return fail(OT_ERR_HIP, "scratch allocation failed");
        ot_status st = compact(n, SpPred{xyz, best, thr}, SpEmit{xyz, inliers, g, stride}, stream, &k, Slot::OP_COMPACT);
        if (st != OT_OK) return st;
        if (k > 0) {
            st = sp_chain_sums(g, stride, k, 3, ws, sums, stream);
            if (st != OT_OK) return st;
            const double kd = (double)k;
            hipLaunchKernelGGL(k_sp_moments, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, stream, (const double*)g,
                               k, stride, sums[0] / kd, sums[1] / kd, sums[2] / kd, prod);
            OT_LAUNCH_CHECK();
            st = sp_chain_sums(prod, stride, k, 6, ws, sums + 3, stream);
            if (st != OT_OK) return st;
        }
    }
    const double kd = (double)k;
    const double ctr[3] = {sums[0] / kd, sums[1] / kd, sums[2] / kd};  // no inliers: 0 / 0, as the definition has it
    plane_from_moments(ctr, sums[3], sums[4], sums[5], sums[6], sums[7], sums[8], plane_host);
    g_sp_times.final_ms = ms_since(t_final);
    *n_inliers_host = k;
    if (evaluated_host) *evaluated_host = (int32_t)count;
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_segment_plane(const double* xyz, int64_t n, double distance_threshold, int32_t ransac_n,
                           int32_t num_iterations, double probability, uint64_t seed, double plane_host[4],
                           int64_t* inliers, int64_t* n_inliers_host, int32_t* evaluated_host, void* stream_) {
    if (!(probability > 0.0 && probability <= 1.0))
        return fail(OT_ERR_INVALID_ARGUMENT, "Probability must be > 0 and <= 1.0");
    if (ransac_n < 3) return fail(OT_ERR_INVALID_ARGUMENT, "ransac_n should be set to higher than or equal to 3.");
    if (n < (int64_t)ransac_n) return fail(OT_ERR_INVALID_ARGUMENT, "There must be at least 'ransac_n' points.");
    if (ransac_n > SP_MAX_RANSAC_N)
        return fail(OT_ERR_INVALID_ARGUMENT, "[SegmentPlane] ransac_n > 32 is not supported by this build");
    if (!xyz || !plane_host || !inliers || !n_inliers_host || n > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, "[SegmentPlane] invalid buffers");
    return segment_plane_run(xyz, n, distance_threshold, ransac_n, num_iterations, probability,
                             (unsigned long long)seed, plane_host, inliers, n_inliers_host, evaluated_host,
                             S(stream_));
}

// test hook (not part of the drop-in boundary): iterations per round trip, 1 .. 1024; 0 restores the default
ot_status otx_segment_plane_chunk(int32_t chunk) {
    if (chunk < 0 || chunk > SP_CHUNK_MAX) return fail(OT_ERR_INVALID_ARGUMENT, "[SegmentPlane] chunk out of range");
    g_sp_chunk = chunk == 0 ? SP_CHUNK : chunk;
    return OT_OK;
}

// test hook (not part of the drop-in boundary): on != 0 times the calling thread's next calls; out8 (nullable, host)
// receives the last call's {count kernels (events), loop wall, tie-break wall, refit chains (events), final pass
// wall} in ms, then chunks, holders of the best count, iterations counted
ot_status otx_segment_plane_profile(int32_t on, double* out8) {
    g_sp_prof = on != 0;
    if (out8) std::memcpy(out8, &g_sp_times, sizeof(double) * 8);
    return OT_OK;
}

}  // extern "C"
