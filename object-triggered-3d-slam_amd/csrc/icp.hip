// icp.hip — PointCloud::Transform and pipelines::registration (EvaluateRegistration, RegistrationICP with
// TransformationEstimationPointToPoint) on MI355X (eval_cone.py:89-97; the definition built against: DESIGN.md §4).
//
// The target is binned once per call into the density-sized grid of ComputePointCloudDistance (grid.h).  One ICP
// iteration is two launches and no host round trip:
//   k_icp_search : one lane per source point.  Moves the kept point by the previous fit's update, finds its nearest
//                  target point within r (rings of cells around the point clamped into the target's box, at most
//                  ceil(r / h) of them; best = the lexicographic minimum of (d2, target index)), writes d2 and the
//                  index (-1: none) and reduces 17 sums over the workgroup's pairs -- k, sum d2, sum (p - c),
//                  sum (q - c), sum (p - c)(q - c)^T about the fixed pivot c (the target box's centre) -- in a fixed
//                  order: lane butterfly, then LDS, then one partial record per workgroup.  No floating-point atomics.
//   k_icp_solve  : one workgroup.  Sums the partials in index order, fitness and rmse, the convergence test against
//                  the previous evaluation, then umeyama's rotation from a one-sided Jacobi SVD of the 3x3 covariance,
//                  update and T = update T into the state record.
// The host queues ICP_CHUNK (search, solve) pairs at a time, one chunk ahead of the one it waits for; a chunk's last
// solve mails the state record to pinned host memory (mail_wait).  Once `done` is set the remaining launches return
// at their first instruction.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "compact.h"
#include "grid.h"
#include "tsdf.h"  // mail_wait

namespace ot {

// Pairs per chunk.  A launch costs the host ~3.5 us and a dependent kernel boundary ~1.5 us, so a chunk of 8 pairs is
// ~55 us of host work against >= 8 searches on the device: the host stays ahead.  With one chunk queued ahead the
// device never waits for the mail's round trip, and a run that stops wastes at most 2 * ICP_CHUNK - 1 pairs of
// launches that return at once (~3 us each).  The reference's runs converge in 5-40 iterations.
constexpr int ICP_CHUNK = 8;
constexpr int ICP_NSUM = 17;  // k, sum d2, sp[3], sq[3], spq[9]
constexpr int ICP_TILE = 128;  // partial records the solve stages in LDS at a time

struct IcpState {
    double T[16];       // accumulated transformation (row-major)
    double update[16];  // the last fit, applied to the kept cloud by the next search
    double fitness, rmse;
    long long k;
    int iter;  // fits performed
    int done;
};
constexpr int ICP_MAIL_WORDS = (int)(sizeof(IcpState) / 4);  // the record, then its sequence word

struct Xform {
    double m[16];
};

// PointCloud::Transform per point: Eigen's column-order 4x4 product, then the perspective division
__device__ inline void xform_point(const double* __restrict__ T, const double p[3], double o[3]) {
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = ((T[r * 4 + 0] * p[0] + T[r * 4 + 1] * p[1]) + T[r * 4 + 2] * p[2]) + T[r * 4 + 3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = v[a] / v[3];
}

// (no __restrict__: the outputs may be the inputs; a lane reads its row before it writes it)
__global__ __launch_bounds__(256) void k_transform(const double* xyz, const double* nrm, int64_t n, Xform T,
                                                   double* out_xyz, double* out_nrm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
    double o[3];
    xform_point(T.m, p, o);
    out_xyz[i * 3] = o[0];
    out_xyz[i * 3 + 1] = o[1];
    out_xyz[i * 3 + 2] = o[2];
    if (nrm) {
        const double v[3] = {nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
            out_nrm[i * 3 + r] = (T.m[r * 4 + 0] * v[0] + T.m[r * 4 + 1] * v[1]) + T.m[r * 4 + 2] * v[2];
    }
}

struct IcpBox {
    double lo[3], hi[3], c[3];
};

// candidates [beg, end) of the sorted target: the lexicographic minimum of (d2, original index) below the start value
__device__ inline void icp_scan(const GridDev& g, const double q[3], int beg, int end, double r2, double& best,
                                int& bi, int& bm) {
    for (int m = beg; m < end; ++m) {
        const double d = d2_l2(q, g.sxyz + (int64_t)m * 3);
        if (d < r2 && d <= best) {
            const int oi = (int)g.sidx[m];
            if (d < best || oi < bi) {
                best = d;
                bi = oi;
                bm = m;
            }
        }
    }
}

// conservative squared gap between a point somewhere in cell 0 and the cells at signed offset d of one axis
__device__ inline double icp_gap(int d, double h) {
    const int a = d < 0 ? -d : d;
    return a > 1 ? (double)(a - 1) * h * (1.0 - 1e-6) : 0.0;
}

__global__ __launch_bounds__(256) void k_icp_search(GridDev g, double* __restrict__ pcd, int64_t n, double r2,
                                                    int rings, IcpBox box, const IcpState* __restrict__ st, int apply,
                                                    double* __restrict__ d2out, int* __restrict__ idxout,
                                                    double* __restrict__ part) {
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[ICP_NSUM];
#pragma unroll
    for (int t = 0; t < ICP_NSUM; ++t) s[t] = 0.0;
    if (i < n) {
        double q[3] = {pcd[i * 3], pcd[i * 3 + 1], pcd[i * 3 + 2]};
        if (apply) {
            double o[3];
            xform_point(st->update, q, o);
#pragma unroll
            for (int a = 0; a < 3; ++a) pcd[i * 3 + a] = q[a] = o[a];
        }
        double qc[3], off2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            qc[a] = fmin(fmax(q[a], box.lo[a]), box.hi[a]);
            const double dd = q[a] - qc[a];
            off2 += dd * dd;
        }
        off2 *= (1.0 - 1e-9);  // a lower bound of |q - p|^2 - |qc - p|^2 for every target p (all inside the box)
        double best = r2;
        int bi = -1, bm = -1;
        if (off2 < r2) {  // NaN coordinates fail this and match nothing
            const int cx = cell_coord(qc[0], g.origin[0], g.h), cy = cell_coord(qc[1], g.origin[1], g.h),
                      cz = cell_coord(qc[2], g.origin[2], g.h);
            // rings 0 and 1 together: the 3x3 columns, cells z-1 .. z+1; then one shell per ring.  After ring rho
            // every unscanned target lies >= rho cells from qc: the walk ends once that cannot beat the best.
            for (int rho = 1; rho <= rings; ++rho) {
                for (int dx = -rho; dx <= rho; ++dx)
                    for (int dy = -rho; dy <= rho; ++dy) {
                        const double ex = icp_gap(dx, g.h), ey = icp_gap(dy, g.h);
                        const double e2 = off2 + (ex * ex + ey * ey);
                        if (!(e2 < best)) continue;
                        const bool face = rho == 1 || dx == -rho || dx == rho || dy == -rho || dy == rho;
                        const int2 col = grid_column(g, 0, cx + dx, cy + dy);
                        if (col.y == 0) continue;
                        if (face) {
                            const int2 se = column_range(g, col, cz - rho, cz + rho);
                            icp_scan(g, q, se.x, se.y, r2, best, bi, bm);
                        } else {
                            const double ez = icp_gap(rho, g.h);
                            if (!(e2 + ez * ez < best)) continue;
                            const int2 a = column_range(g, col, cz - rho, cz - rho);
                            icp_scan(g, q, a.x, a.y, r2, best, bi, bm);
                            const int2 b = column_range(g, col, cz + rho, cz + rho);
                            icp_scan(g, q, b.x, b.y, r2, best, bi, bm);
                        }
                    }
                const double guard = ((double)rho - 0.01) * g.h;
                if (!(off2 + guard * guard < best)) break;
            }
        }
        d2out[i] = bi >= 0 ? best : -1.0;
        idxout[i] = bi;
        if (bi >= 0) {
            const double* t = g.sxyz + (int64_t)bm * 3;
            const double p[3] = {q[0] - box.c[0], q[1] - box.c[1], q[2] - box.c[2]};
            const double w[3] = {t[0] - box.c[0], t[1] - box.c[1], t[2] - box.c[2]};
            s[0] = 1.0;
            s[1] = best;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[2 + a] = p[a];
                s[5 + a] = w[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) s[8 + a * 3 + b] = p[a] * w[b];
            }
        }
    }
    // fixed-order reduction: the lane butterfly (every lane ends with the same sum), the 4 waves through LDS in wave
    // order, one partial record per workgroup
    __shared__ double ws[4][ICP_NSUM];
#pragma unroll
    for (int t = 0; t < ICP_NSUM; ++t) s[t] = wave_sum(s[t]);
    if (lane_id() == 0)
#pragma unroll
        for (int t = 0; t < ICP_NSUM; ++t) ws[threadIdx.x >> 6][t] = s[t];
    __syncthreads();
    if (threadIdx.x < ICP_NSUM) {
        const int t = threadIdx.x;
        part[(int64_t)blockIdx.x * ICP_NSUM + t] = ((ws[0][t] + ws[1][t]) + ws[2][t]) + ws[3][t];
    }
}

// ---- the fit (one thread) ------------------------------------------------------------------------------------------
__device__ inline double det3(const double a[3][3]) {
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}

// umeyama's rotation R = U diag(1, 1, sign(det U det V)) V^T of the 3x3 covariance A = U D V^T.  One-sided Jacobi:
// column rotations of A (accumulated in V) until its columns are orthogonal; their norms are the singular values and
// their directions U's columns.  The third column of U is +-(u0 x u1), its sign from the third column of A V: exact
// for a singular A too (planar or collinear pairs), where that column carries no direction.
__device__ inline void umeyama_rotation(const double Ain[3][3], double R[3][3]) {
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[i][j] = Ain[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < 3; ++i) {
                    al += A[i][p] * A[i][p];
                    be += A[i][q] * A[i][q];
                    ga += A[i][p] * A[i][q];
                }
                if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double sg[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) sg[j] = sqrt((A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j]);
    for (int a = 0; a < 2; ++a)  // singular values in decreasing order (the sign goes to the smallest)
        for (int b = 0; b < 2 - a; ++b)
            if (sg[ord[b]] < sg[ord[b + 1]]) {
                const int t = ord[b];
                ord[b] = ord[b + 1];
                ord[b + 1] = t;
            }
    double U[3][3], W[3][3];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) W[i][j] = V[i][ord[j]];
    const double s0 = sg[ord[0]], s1 = sg[ord[1]];
    if (!(s0 > 0.0)) {  // A = 0 (one pair, or all pairs at one point): Eigen's U = V = I
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
        return;
    }
    for (int i = 0; i < 3; ++i) U[i][0] = A[i][ord[0]] / s0;
    if (s1 > 1e-14 * s0) {
        double d = 0.0;  // one Gram-Schmidt step against u0 keeps U orthonormal when s1 is small
        for (int i = 0; i < 3; ++i) d += A[i][ord[1]] * U[i][0];
        double nn = 0.0;
        for (int i = 0; i < 3; ++i) {
            U[i][1] = A[i][ord[1]] - d * U[i][0];
            nn += U[i][1] * U[i][1];
        }
        nn = sqrt(nn);
        for (int i = 0; i < 3; ++i) U[i][1] /= nn;
    } else {  // rank 1: any unit vector orthogonal to u0 (from the axis u0 is least aligned with)
        int m = 0;
        for (int i = 1; i < 3; ++i)
            if (fabs(U[i][0]) < fabs(U[m][0])) m = i;
        double e[3] = {0.0, 0.0, 0.0};
        e[m] = 1.0;
        const double d = U[m][0];
        double nn = 0.0;
        for (int i = 0; i < 3; ++i) {
            U[i][1] = e[i] - d * U[i][0];
            nn += U[i][1] * U[i][1];
        }
        nn = sqrt(nn);
        for (int i = 0; i < 3; ++i) U[i][1] /= nn;
    }
    const double cr[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1],
                          U[0][0] * U[1][1] - U[1][0] * U[0][1]};
    const double dir = (cr[0] * A[0][ord[2]] + cr[1] * A[1][ord[2]]) + cr[2] * A[2][ord[2]];
    const double su = dir < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i) U[i][2] = su * cr[i];
    const double sgn = det3(U) * det3(W) < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = (U[i][0] * W[j][0] + U[i][1] * W[j][1]) + sgn * U[i][2] * W[j][2];
}

// seq != 0: this solve ends a chunk and mails the record (plain vector stores to coherent host memory, then seq)
__global__ __launch_bounds__(256) void k_icp_solve(const double* __restrict__ part, int nblocks, int64_t n, IcpBox box,
                                                  double rel_fitness, double rel_rmse, int max_iteration,
                                                  IcpState* st, unsigned* mail, unsigned seq) {
    __shared__ double sum[ICP_NSUM];
    __shared__ double tile[ICP_TILE * ICP_NSUM];
    __shared__ int was_done;
    if (threadIdx.x == 0) was_done = st->done;
    __syncthreads();
    if (!was_done) {
        // the partials in index order: ICP_TILE records at a time land in LDS through all lanes' loads (one lane
        // walking global memory paid a load's latency per record: 57 us for 196 records), then lane t adds component t
        double a = 0.0;
        for (int base = 0; base < nblocks; base += ICP_TILE) {
            const int cnt = min(ICP_TILE, nblocks - base) * ICP_NSUM;
            for (int e = threadIdx.x; e < cnt; e += 256) tile[e] = part[(int64_t)base * ICP_NSUM + e];
            __syncthreads();
            if (threadIdx.x < ICP_NSUM)
                for (int e = threadIdx.x; e < cnt; e += ICP_NSUM) a += tile[e];
            __syncthreads();
        }
        if (threadIdx.x < ICP_NSUM) sum[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double k = sum[0];
            const double fitness = k > 0.0 ? k / (double)n : 0.0;
            const double rmse = k > 0.0 ? sqrt(sum[1] / k) : 0.0;
            const int iter = st->iter;
            const bool conv = iter > 0 && fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse;
            st->fitness = fitness;
            st->rmse = rmse;
            st->k = (long long)k;
            if (conv || iter >= max_iteration) {
                st->done = 1;
            } else {
                double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, t[3] = {0.0, 0.0, 0.0};
                if (k > 0.0) {
                    double mp[3], mq[3], C[3][3];
                    for (int a = 0; a < 3; ++a) {
                        mp[a] = sum[2 + a] / k;
                        mq[a] = sum[5 + a] / k;
                    }
                    for (int a = 0; a < 3; ++a)  // sigma = (1/k) sum (q - mq)(p - mp)^T, rows q, columns p
                        for (int b = 0; b < 3; ++b) C[a][b] = sum[8 + b * 3 + a] / k - mq[a] * mp[b];
                    umeyama_rotation(C, R);
                    for (int a = 0; a < 3; ++a) {
                        const double mup[3] = {mp[0] + box.c[0], mp[1] + box.c[1], mp[2] + box.c[2]};
                        t[a] = (mq[a] + box.c[a]) - ((R[a][0] * mup[0] + R[a][1] * mup[1]) + R[a][2] * mup[2]);
                    }
                }
                double up[16], Tn[16];
                for (int a = 0; a < 3; ++a) {
                    for (int b = 0; b < 3; ++b) up[a * 4 + b] = R[a][b];
                    up[a * 4 + 3] = t[a];
                }
                up[12] = up[13] = up[14] = 0.0;
                up[15] = 1.0;
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b)
                        Tn[a * 4 + b] = ((up[a * 4 + 0] * st->T[0 * 4 + b] + up[a * 4 + 1] * st->T[1 * 4 + b]) +
                                         up[a * 4 + 2] * st->T[2 * 4 + b]) + up[a * 4 + 3] * st->T[3 * 4 + b];
                for (int e = 0; e < 16; ++e) {
                    st->update[e] = up[e];
                    st->T[e] = Tn[e];
                }
                st->iter = iter + 1;
            }
        }
        __syncthreads();
    }
    if (seq) {
        __threadfence();
        const unsigned* w = (const unsigned*)st;
        for (int e = threadIdx.x; e < ICP_MAIL_WORDS; e += 256) mail[e] = w[e];
        __threadfence_system();  // the record reaches the host before its sequence word
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(mail + ICP_MAIL_WORDS, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct CorrPred {
    const int* idx;
    __device__ bool operator()(int64_t i) const { return idx[i] >= 0; }
};
struct CorrEmit {
    const int* idx;
    int32_t* corr;
    __device__ void operator()(int64_t i, int64_t pos) const {
        corr[pos * 2] = (int32_t)i;
        corr[pos * 2 + 1] = idx[i];
    }
};

static thread_local unsigned g_icp_seq = 0;
// test hook otx_registration_last_d2: the last call's per-source-point d2 (-1: no correspondence)
static thread_local const double* g_icp_d2 = nullptr;
static thread_local int64_t g_icp_d2_n = 0;

static bool is_identity(const double* T) {
    for (int e = 0; e < 16; ++e)
        if (T[e] != ((e % 5) == 0 ? 1.0 : 0.0)) return false;
    return true;
}

// evaluate (max_iteration == 0, always_transform) or the ICP loop; outputs as in otslam.h
static ot_status icp_run(const double* src, int64_t n, const double* tgt, int64_t m, double r, const double* init,
                         bool always_transform, double rel_fitness, double rel_rmse, int max_iteration, double* T_out,
                         double* fitness, double* rmse, int32_t* corr, int64_t* n_corr, int32_t* iterations,
                         hipStream_t stream) {
    if (!always_transform && !(r > 0.0)) return fail(OT_ERR_INVALID_ARGUMENT, "Invalid max_correspondence_distance.");
    if (n < 0 || m < 0 || n > 0x7FFFFFFF || m > 0x7FFFFFFF || (n > 0 && !src) || (m > 0 && !tgt) || !init)
        return fail(OT_ERR_INVALID_ARGUMENT, "[RegistrationICP] invalid buffers");
    if (T_out) std::memcpy(T_out, init, sizeof(double) * 16);
    if (fitness) *fitness = 0.0;
    if (rmse) *rmse = 0.0;
    if (n_corr) *n_corr = 0;
    if (iterations) *iterations = 0;
    g_icp_d2 = nullptr;
    g_icp_d2_n = 0;
    if (n == 0 || m == 0 || !(r > 0.0)) return OT_OK;  // (EvaluateRegistration with r <= 0: no radius, no pairs)
    if (max_iteration < 0) max_iteration = 0;

    IcpBox box;
    GridBuild gb;
    ot_status st = nn_target_grid(tgt, m, 0, stream, box.lo, box.hi, gb);
    if (st != OT_OK) return st;
    for (int a = 0; a < 3; ++a) box.c[a] = 0.5 * (box.lo[a] + box.hi[a]);
    // two points closer than r lie at most ceil(r / h) cells apart per axis (the margin covers the rounding of the
    // cell coordinates); a ring past the grid's longest axis holds no cell
    const int rings = (int)std::min(std::ceil(r / gb.g.h + 1e-6),
                                    (double)std::max(gb.g.dim[0], std::max(gb.g.dim[1], gb.g.dim[2])));

    const int nblocks = (int)((n + 255) / 256);
    double* pcd = (double*)scratch((size_t)n * 24 + 64, Slot::ICP_PCD);
    double *d2, *part;  // (plain pointers: the iteration lambda below captures them)
    int* idx;
    IcpState* dst;
    std::tie(d2, idx) = carve(scratch_of(Slot::ICP_NN), Arr<double>{(size_t)n}, Arr<int>{(size_t)n});
    std::tie(dst, part) =
        carve(scratch_of(Slot::ICP_PARTIALS), Arr<IcpState>{1}, Arr<double>{(size_t)nblocks * ICP_NSUM});
    unsigned* mail = (unsigned*)pinned_scratch(2 * 4 * (ICP_MAIL_WORDS + 2), PinnedSlot::ICP_MAIL, true);
    if (!pcd || !d2 || !dst || !mail) return fail(OT_ERR_HIP, "scratch allocation failed");
    unsigned* mbox[2] = {mail, mail + ICP_MAIL_WORDS + 2};
    mbox[0][ICP_MAIL_WORDS] = 0;  // sequence words start below every seq sent (nothing of an earlier call is in flight)
    mbox[1][ICP_MAIL_WORDS] = 0;

    IcpState h0;
    std::memset(&h0, 0, sizeof(h0));
    std::memcpy(h0.T, init, sizeof(double) * 16);
    for (int e = 0; e < 16; e += 5) h0.update[e] = 1.0;
    st = upload_small(dst, &h0, sizeof(h0), stream);
    if (st != OT_OK) return st;
    if (always_transform || !is_identity(init)) {
        Xform X;
        std::memcpy(X.m, init, sizeof(X.m));
        hipLaunchKernelGGL(k_transform, dim3((unsigned)nblocks), dim3(256), 0, stream, src, (const double*)nullptr, n,
                           X, pcd, (double*)nullptr);
        OT_LAUNCH_CHECK();
    } else {
        OT_HIP_TRY(hipMemcpyAsync(pcd, src, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, stream));
    }

    const double r2 = r * r;
    const int total = max_iteration + 1;  // evaluations: the first, then one per fit
    auto enqueue = [&](int first, int count, unsigned seq, unsigned* box_mail) -> ot_status {
        for (int j = first; j < first + count; ++j) {
            hipLaunchKernelGGL(k_icp_search, dim3((unsigned)nblocks), dim3(256), 0, stream, gb.g, pcd, n, r2, rings, box,
                               (const IcpState*)dst, j > 0 ? 1 : 0, d2, idx, part);
            hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(256), 0, stream, (const double*)part, nblocks, n, box,
                               rel_fitness, rel_rmse, max_iteration, dst, box_mail, j == first + count - 1 ? seq : 0u);
        }
        OT_LAUNCH_CHECK();
        return OT_OK;
    };
    IcpState hs;
    std::memset(&hs, 0, sizeof(hs));
    int queued = 0, chunk = 0;
    unsigned seqs[2] = {0, 0};
    auto queue_chunk = [&]() -> ot_status {
        const int count = std::min(ICP_CHUNK, total - queued);
        if (++g_icp_seq == 0) ++g_icp_seq;  // 0 means "do not mail"
        seqs[chunk & 1] = g_icp_seq;
        ot_status s = enqueue(queued, count, seqs[chunk & 1], mbox[chunk & 1]);
        queued += count;
        ++chunk;
        return s;
    };
    st = queue_chunk();
    if (st != OT_OK) return st;
    for (int waiting = 0;; ++waiting) {  // chunk `waiting` is queued; queue the next before waiting for it
        if (queued < total) {
            st = queue_chunk();
            if (st != OT_OK) return st;
        }
        st = mail_wait(mbox[waiting & 1] + ICP_MAIL_WORDS, seqs[waiting & 1], stream);
        if (st != OT_OK) return st;
        std::memcpy(&hs, mbox[waiting & 1], sizeof(hs));
        if (hs.done || waiting + 1 >= chunk) break;
    }
    if (!hs.done) return fail(OT_ERR_HIP, "[RegistrationICP] the iteration chain ended without a result");
    g_icp_d2 = d2;
    g_icp_d2_n = n;
    if (T_out) std::memcpy(T_out, hs.T, sizeof(double) * 16);
    if (fitness) *fitness = hs.fitness;
    if (rmse) *rmse = hs.rmse;
    if (iterations) *iterations = hs.iter;
    if (n_corr) *n_corr = hs.k;
    if (corr) {
        int64_t k = 0;
        st = compact(n, CorrPred{idx}, CorrEmit{idx, corr}, stream, &k, Slot::OP_COMPACT);  // synchronises
        if (st != OT_OK) return st;
        if (n_corr) *n_corr = k;
    } else {
        OT_HIP_TRY(hipStreamSynchronize(stream));  // the launches queued past `done` have drained
    }
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_transform_points(const double* xyz, const double* normals, int64_t n, const double T_host[16],
                              double* out_xyz, double* out_normals, void* stream_) {
    hipStream_t stream = S(stream_);
    if (n < 0 || !T_host) return fail(OT_ERR_INVALID_ARGUMENT, "[Transform] invalid arguments");
    if (n == 0) return OT_OK;
    if (!xyz || !out_xyz || (normals && !out_normals) || n > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, "[Transform] invalid buffers");
    Xform X;
    std::memcpy(X.m, T_host, sizeof(X.m));
    hipLaunchKernelGGL(k_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xyz, normals, n, X, out_xyz,
                       out_normals);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

ot_status ot_evaluate_registration(const double* src, int64_t n, const double* tgt, int64_t m, double max_corr_dist,
                                   const double T_host[16], double* fitness_host, double* rmse_host, int32_t* corr,
                                   int64_t* n_corr_host, void* stream_) {
    return icp_run(src, n, tgt, m, max_corr_dist, T_host, true, 0.0, 0.0, 0, nullptr, fitness_host, rmse_host, corr,
                   n_corr_host, nullptr, S(stream_));
}

ot_status ot_registration_icp(const double* src, int64_t n, const double* tgt, int64_t m, double max_corr_dist,
                              const double init_host[16], double relative_fitness, double relative_rmse,
                              int32_t max_iteration, double T_out_host[16], double* fitness_host, double* rmse_host,
                              int32_t* corr, int64_t* n_corr_host, int32_t* iterations_host, void* stream_) {
    return icp_run(src, n, tgt, m, max_corr_dist, init_host, false, relative_fitness, relative_rmse, max_iteration,
                   T_out_host, fitness_host, rmse_host, corr, n_corr_host, iterations_host, S(stream_));
}

// test hook (not part of the drop-in boundary): the squared distances of the calling thread's last evaluation, one per
// source point (-1: no correspondence), copied to out (device, n doubles)
ot_status otx_registration_last_d2(double* out, int64_t n, void* stream_) {
    if (!out || n != g_icp_d2_n || !g_icp_d2) return fail(OT_ERR_INVALID_ARGUMENT, "no evaluation of that size");
    OT_HIP_TRY(hipMemcpyAsync(out, g_icp_d2, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, S(stream_)));
    OT_HIP_TRY(hipStreamSynchronize(S(stream_)));
    return OT_OK;
}

}  // extern "C"
