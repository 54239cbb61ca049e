// normals.hip — PointCloud::EstimateCovariances / EstimateNormals (fast_normal_computation), the two closed-form
// normal orientations and NormalizeNormals on MI355X ("normals").
//
// Neighbours come from the uniform cell grid of grid.h, sized as SOR sizes it (sor_cell_target).  The result is
// defined by the distances and the point indices alone: the first k points in ascending (d2, index) order, so the
// grid only decides which candidates a query scans.
//   k_nrm_cov      : one lane per query in the grid's sorted cell order.  The lane finds its sorted (d2, index) list
//                    in LDS (nb_list.h: the search, shared with features.hip), then gathers the neighbours in list
//                    order for the nine sequential sums (the order is the result).
//   k_nrm_from_cov : one lane per point: Open3D's FastEigen3x3 on the covariance, the zero-normal and prior rules.
//   k_nrm_orient / k_nrm_normalize : elementwise.
// Everything is float64 without contraction; acos and cos (device library) are the only operations whose last bits
// may differ from a host restatement.
#include <algorithm>
#include <cmath>

#include "nb_list.h"
#include "sor.h"

namespace ot {

// r2 <= 0: KNN; r2 > 0: hybrid (the first kk, of these the ones with d2 < r2)
template <int KMAX>
__global__ __launch_bounds__(64) void k_nrm_cov(GridDev g, const double* __restrict__ xyz, int64_t n, int k, double r2,
                                                double* __restrict__ cov) {
    __shared__ double s_d[KMAX * 64];
    __shared__ unsigned s_i[KMAX * 64];
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    double* Ld = s_d + threadIdx.x;
    unsigned* Li = s_i + threadIdx.x;
    const int kk = (int)((int64_t)k < n ? k : n);  // <= KMAX (host)
    const int m = nb_search(g, n, j, kk, r2, Ld, Li);
    double* C = cov + (int64_t)g.sidx[j] * 9;
    if (m < 3) {
        C[0] = 1.0, C[1] = 0.0, C[2] = 0.0;
        C[3] = 0.0, C[4] = 1.0, C[5] = 0.0;
        C[6] = 0.0, C[7] = 0.0, C[8] = 1.0;
        return;
    }
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < m; ++t) {
        const double* p = xyz + (int64_t)Li[t * 64] * 3;
        const double x = p[0], y = p[1], z = p[2];
        s[0] += x;
        s[1] += y;
        s[2] += z;
        s[3] += x * x;
        s[4] += x * y;
        s[5] += x * z;
        s[6] += y * y;
        s[7] += y * z;
        s[8] += z * z;
    }
    const double dm = (double)m;
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = s[t] / dm;
    const double c01 = s[4] - s[0] * s[1], c02 = s[5] - s[0] * s[2], c12 = s[7] - s[1] * s[2];
    C[0] = s[3] - s[0] * s[0];
    C[1] = c01;
    C[2] = c02;
    C[3] = c01;
    C[4] = s[6] - s[1] * s[1];
    C[5] = c12;
    C[6] = c02;
    C[7] = c12;
    C[8] = s[8] - s[2] * s[2];
}

// ------------------------------------------------------------------------------------------ FastEigen3x3
struct V3 {
    double x, y, z;
};
__device__ inline V3 cross3(V3 a, V3 b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ inline double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

struct Sym3 {
    double a00, a01, a02, a11, a12, a22;
};

// eigenvector of the well-separated eigenvalue e: the longest cross product of two rows of A - e I, normalised
__device__ inline V3 eigvec0(const Sym3& A, double e) {
    const V3 r0{A.a00 - e, A.a01, A.a02}, r1{A.a01, A.a11 - e, A.a12}, r2{A.a02, A.a12, A.a22 - e};
    const V3 c0 = cross3(r0, r1), c1 = cross3(r0, r2), c2 = cross3(r1, r2);
    const double d0 = dot3(c0, c0), d1 = dot3(c1, c1), d2 = dot3(c2, c2);
    V3 c = c0;
    double dm = d0;
    if (d1 > dm) {
        dm = d1;
        c = c1;
    }
    if (d2 > dm) {
        dm = d2;
        c = c2;
    }
    const double s = sqrt(dm);
    return V3{c.x / s, c.y / s, c.z / s};
}

// eigenvector of e1 in the plane orthogonal to v0
__device__ inline V3 eigvec1(const Sym3& A, V3 v0, double e1) {
    V3 U;
    if (fabs(v0.x) > fabs(v0.y)) {
        const double inv = 1.0 / sqrt(v0.x * v0.x + v0.z * v0.z);
        U = V3{-v0.z * inv, 0.0, v0.x * inv};
    } else {
        const double inv = 1.0 / sqrt(v0.y * v0.y + v0.z * v0.z);
        U = V3{0.0, v0.z * inv, -v0.y * inv};
    }
    const V3 W = cross3(v0, U);
    const V3 a0{A.a00, A.a01, A.a02}, a1{A.a01, A.a11, A.a12}, a2{A.a02, A.a12, A.a22};
    const V3 AU{dot3(a0, U), dot3(a1, U), dot3(a2, U)}, AW{dot3(a0, W), dot3(a1, W), dot3(a2, W)};
    double m00 = dot3(U, AU) - e1, m01 = dot3(U, AW), m11 = dot3(W, AW) - e1;
    const double b00 = fabs(m00), b01 = fabs(m01), b11 = fabs(m11);
    if (b00 >= b11) {
        if (!((b00 > b01 ? b00 : b01) > 0.0)) return U;
        if (b00 >= b01) {
            m01 = m01 / m00;
            m00 = 1.0 / sqrt(1.0 + m01 * m01);
            m01 = m01 * m00;
        } else {
            m00 = m00 / m01;
            m01 = 1.0 / sqrt(1.0 + m00 * m00);
            m00 = m00 * m01;
        }
        return V3{m01 * U.x - m00 * W.x, m01 * U.y - m00 * W.y, m01 * U.z - m00 * W.z};
    }
    if (!((b11 > b01 ? b11 : b01) > 0.0)) return U;
    if (b11 >= b01) {
        m01 = m01 / m11;
        m11 = 1.0 / sqrt(1.0 + m01 * m01);
        m01 = m01 * m11;
    } else {
        m11 = m11 / m01;
        m01 = 1.0 / sqrt(1.0 + m11 * m11);
        m11 = m11 * m01;
    }
    return V3{m11 * U.x - m01 * W.x, m11 * U.y - m01 * W.y, m11 * U.z - m01 * W.z};
}

// the eigenvector of the smallest eigenvalue of the symmetric C (row-major [9]); zero for a zero matrix
__device__ inline V3 fast_eigen3(const double* C) {
    const double c[6] = {C[0], C[1], C[2], C[4], C[5], C[8]};
    double mx = c[0];
#pragma unroll
    for (int t = 1; t < 6; ++t)
        if (c[t] > mx) mx = c[t];
    if (mx == 0.0) return V3{0.0, 0.0, 0.0};
    const Sym3 A{c[0] / mx, c[1] / mx, c[2] / mx, c[3] / mx, c[4] / mx, c[5] / mx};
    const double norm = (A.a01 * A.a01 + A.a02 * A.a02) + A.a12 * A.a12;
    if (!(norm > 0.0)) {  // diagonal
        if (A.a00 < A.a11 && A.a00 < A.a22) return V3{1.0, 0.0, 0.0};
        if (A.a11 < A.a00 && A.a11 < A.a22) return V3{0.0, 1.0, 0.0};
        return V3{0.0, 0.0, 1.0};
    }
    const double q = ((A.a00 + A.a11) + A.a22) / 3.0;
    const double b00 = A.a00 - q, b11 = A.a11 - q, b22 = A.a22 - q;
    const double p = sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + norm * 2.0) / 6.0);
    const double c00 = b11 * b22 - A.a12 * A.a12;
    const double c01 = A.a01 * b22 - A.a12 * A.a02;
    const double c02 = A.a01 * A.a12 - b11 * A.a02;
    const double det = ((b00 * c00 - A.a01 * c01) + A.a02 * c02) / ((p * p) * p);
    double hd = det * 0.5;
    if (hd < -1.0) hd = -1.0;
    if (hd > 1.0) hd = 1.0;
    const double ang = acos(hd) / 3.0;
    const double beta2 = cos(ang) * 2.0;
    const double beta0 = cos(ang + 2.09439510239319549) * 2.0;
    const double beta1 = -(beta0 + beta2);
    const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;
    if (hd >= 0.0) {
        const V3 v2 = eigvec0(A, e2);
        if (e2 < e0 && e2 < e1) return v2;
        const V3 v1 = eigvec1(A, v2, e1);
        if (e1 < e0 && e1 < e2) return v1;
        return cross3(v1, v2);
    }
    const V3 v0 = eigvec0(A, e0);
    if (e0 < e1 && e0 < e2) return v0;
    const V3 v1 = eigvec1(A, v0, e1);
    if (e1 < e0 && e1 < e2) return v1;
    return cross3(v0, v1);
}

// prior (nullable) may alias out: a lane reads its own row before it writes it
__global__ __launch_bounds__(256) void k_nrm_from_cov(const double* __restrict__ cov, int64_t n, const double* prior,
                                                      double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    V3 v = fast_eigen3(cov + i * 9);
    V3 old{0.0, 0.0, 1.0};
    if (prior) old = V3{prior[i * 3], prior[i * 3 + 1], prior[i * 3 + 2]};
    if (dot3(v, v) == 0.0) v = old;
    if (prior && dot3(v, old) < 0.0) v = V3{-v.x, -v.y, -v.z};
    out[i * 3] = v.x;
    out[i * 3 + 1] = v.y;
    out[i * 3 + 2] = v.z;
}

// mode 0: the reference vector is ref; mode 1: ref - xyz[i]
__global__ __launch_bounds__(256) void k_nrm_orient(double* __restrict__ nrm, const double* __restrict__ xyz,
                                                    int64_t n, int mode, double rx, double ry, double rz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    V3 v{nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2]};
    V3 ref{rx, ry, rz};
    if (mode == 1) ref = V3{rx - xyz[i * 3], ry - xyz[i * 3 + 1], rz - xyz[i * 3 + 2]};
    if (dot3(v, v) == 0.0) {
        v = ref;
        if (mode == 1) {
            const double sq = dot3(ref, ref);
            if (sq == 0.0) {
                v = V3{0.0, 0.0, 1.0};
            } else {
                const double s = sqrt(sq);
                v = V3{ref.x / s, ref.y / s, ref.z / s};
            }
        }
    } else if (dot3(v, ref) < 0.0) {
        v = V3{-v.x, -v.y, -v.z};
    }
    nrm[i * 3] = v.x;
    nrm[i * 3 + 1] = v.y;
    nrm[i * 3 + 2] = v.z;
}

__global__ __launch_bounds__(256) void k_nrm_normalize(double* __restrict__ nrm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const V3 v{nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2]};
    const double sq = dot3(v, v);
    if (!(sq > 0.0)) return;
    const double s = sqrt(sq);
    nrm[i * 3] = v.x / s;
    nrm[i * 3 + 1] = v.y / s;
    nrm[i * 3 + 2] = v.z / s;
}

static ot_status check_search(const char* who, int32_t knn, double radius) {
    if (knn < 1 || knn > 64)
        return fail(OT_ERR_INVALID_ARGUMENT, std::string(who) + " knn / max_nn must lie in 1..64 (the neighbour list "
                                                                "is kept on chip), got " + std::to_string(knn));
    if (std::isnan(radius)) return fail(OT_ERR_INVALID_ARGUMENT, std::string(who) + " radius is NaN");
    return OT_OK;
}

// cov[n][9] of the cloud (n > 0); synchronises (grid build), the kernel itself is only queued
static ot_status covariances(const double* xyz, int64_t n, int32_t knn, double radius, double* cov,
                             hipStream_t stream) {
    // cells sized as SOR's (sor.h): the grid only changes speed
    double mn[3], mx[3];
    GridBuild gb;
    ot_status st = occupancy_grid(xyz, n, sor_cell_target(knn), GRID_NBR3, mn, mx, stream, gb);
    if (st != OT_OK) return st;
    const double r2 = radius > 0.0 ? radius * radius : 0.0;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (knn <= 32) hipLaunchKernelGGL(k_nrm_cov<32>, grid, block, 0, stream, gb.g, xyz, n, (int)knn, r2, cov);
    else hipLaunchKernelGGL(k_nrm_cov<64>, grid, block, 0, stream, gb.g, xyz, n, (int)knn, r2, cov);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_estimate_covariances(const double* xyz, int64_t n, int32_t knn, double radius, double* cov_out,
                                  void* stream_) {
    hipStream_t stream = S(stream_);
    ot_status st = check_search("[EstimateCovariances]", knn, radius);
    if (st != OT_OK) return st;
    if (n <= 0) return OT_OK;
    if (!xyz || !cov_out || n > 0x7FFFFFFF) return fail(OT_ERR_INVALID_ARGUMENT, "[EstimateCovariances] invalid buffers");
    st = covariances(xyz, n, knn, radius, cov_out, stream);
    if (st != OT_OK) return st;
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_estimate_normals(const double* xyz, int64_t n, int32_t knn, double radius, const double* prior_normals,
                              double* normals_out, double* cov_out, void* stream_) {
    hipStream_t stream = S(stream_);
    ot_status st = check_search("[EstimateNormals]", knn, radius);
    if (st != OT_OK) return st;
    if (n <= 0) return OT_OK;
    if (!xyz || !normals_out || n > 0x7FFFFFFF) return fail(OT_ERR_INVALID_ARGUMENT, "[EstimateNormals] invalid buffers");
    double* cov = cov_out;
    if (!cov) {
        cov = (double*)scratch((size_t)n * 9 * sizeof(double), Slot::OP_WS);
        if (!cov) return fail(OT_ERR_HIP, "scratch allocation failed");
    }
    st = covariances(xyz, n, knn, radius, cov, stream);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_nrm_from_cov, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)cov, n,
                       prior_normals, normals_out);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_orient_normals(double* normals_inout, const double* xyz, int64_t n, int32_t mode, const double* ref3_host,
                            void* stream_) {
    hipStream_t stream = S(stream_);
    if (mode != 0 && mode != 1) return fail(OT_ERR_INVALID_ARGUMENT, "[OrientNormals] mode must be 0 or 1");
    if (!ref3_host) return fail(OT_ERR_INVALID_ARGUMENT, "[OrientNormals] the reference vector is NULL");
    if (n <= 0) return OT_OK;
    if (!normals_inout || (mode == 1 && !xyz)) return fail(OT_ERR_INVALID_ARGUMENT, "[OrientNormals] invalid buffers");
    hipLaunchKernelGGL(k_nrm_orient, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, normals_inout, xyz, n,
                       (int)mode, ref3_host[0], ref3_host[1], ref3_host[2]);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

ot_status ot_normalize_normals(double* normals_inout, int64_t n, void* stream_) {
    hipStream_t stream = S(stream_);
    if (n <= 0) return OT_OK;
    if (!normals_inout) return fail(OT_ERR_INVALID_ARGUMENT, "[NormalizeNormals] invalid buffers");
    hipLaunchKernelGGL(k_nrm_normalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, normals_inout, n);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // extern "C"
