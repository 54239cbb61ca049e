// voxel_keys.h — the float64 voxel keys and the in-index-order voxel averages, shared by PointCloud::VoxelDownSample
// (voxel.hip) and TriangleMesh::SimplifyVertexClustering (mesh_filter.hip): one statement of the key formula, of its
// refusals and of the summation chain.  Internal linkage: every translation unit gets its own copy of the kernels.
#pragma once

#include <cmath>

#include "compact.h"

namespace ot {

// width of the packed key on the host (the same float64 formula as k_voxel_keys), so the radix sort runs only the
// passes the key needs
inline int voxel_key_end_bit(const Bounds& hb, double vs) {
    int end_bit = 0;
    for (int a = 0; a < 3; ++a) {
        const double vmin = ordered_to_dbl(hb.mn[a]) - vs * 0.5;
        const double vmax = ordered_to_dbl(hb.mx[a]) + vs * 0.5;
        const double span = std::floor((vmax - vmin) / vs);
        int bits = 1;
        while (bits < 62 && span >= std::ldexp(1.0, bits)) ++bits;
        end_bit += bits;
    }
    return std::min(end_bit, 64);
}

namespace {

// key = floor((p - (min - vs/2)) / vs) per axis in float64, packed x-major with per-axis widths from the extent;
// b->err: 1 = voxel_size is too small (vs * INT_MAX < extent), 2 = the packed key would need more than 64 bits
__global__ __launch_bounds__(256) void k_voxel_keys(const double* __restrict__ xyz, int64_t n, double vs,
                                                    Bounds* b, unsigned long long* keys, unsigned* idx) {
    double vmin[3];
    int bits[3];
    long long kmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vmin[a] = ordered_to_dbl(b->mn[a]) - vs * 0.5;
        const double vmax = ordered_to_dbl(b->mx[a]) + vs * 0.5;
        kmax[a] = (long long)floor((vmax - vmin[a]) / vs);
        bits[a] = bits_for(kmax[a]);
    }
    const double ext = fmax(fmax(ordered_to_dbl(b->mx[0]) + vs * 0.5 - vmin[0], ordered_to_dbl(b->mx[1]) + vs * 0.5 - vmin[1]),
                            ordered_to_dbl(b->mx[2]) + vs * 0.5 - vmin[2]);
    const bool too_small = vs * 2147483647.0 < ext;
    const bool too_wide = bits[0] + bits[1] + bits[2] > 64;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && (too_small || too_wide)) b->err = too_small ? 1 : 2;
    if (i >= n) return;
    long long k[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) k[a] = (long long)(int)floor((xyz[i * 3 + a] - vmin[a]) / vs);
    keys[i] = ((unsigned long long)k[0] << (bits[1] + bits[2])) | ((unsigned long long)k[1] << bits[2]) |
              (unsigned long long)k[2];
    idx[i] = (unsigned)i;
}

// one lane per voxel (a segment of the key-sorted points, heads[s] its start): the sums of its points' rows in index
// order, from 0, divided by the count.  out_row (nullable): voxel s writes row out_row[s] instead of row s.
__global__ __launch_bounds__(256) void k_voxel_reduce(const double* __restrict__ xyz, const double* __restrict__ rgb,
                                                      const double* __restrict__ nrm, const unsigned* __restrict__ sidx,
                                                      const unsigned long long* __restrict__ skeys,
                                                      const int* __restrict__ heads, int64_t K, int64_t n,
                                                      const Bounds* b, double vs, double* oxyz, double* orgb,
                                                      double* onrm, int32_t* okeys, const int* __restrict__ out_row) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= K) return;
    const int64_t beg = heads[s];
    const int64_t end = (s + 1 < K) ? heads[s + 1] : n;
    double p[3] = {0, 0, 0}, c[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    // points in batches of 4: the batch's index and row loads are all issued before its (in-order) sums
    constexpr int VB = 4;
    for (int64_t j0 = beg; j0 < end; j0 += VB) {
        int64_t ii[VB];
#pragma unroll
        for (int k = 0; k < VB; ++k) ii[k] = sidx[j0 + k < end ? j0 + k : j0];
        double xp[VB][3], xc[VB][3], xq[VB][3];
#pragma unroll
        for (int k = 0; k < VB; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                xp[k][a] = xyz[ii[k] * 3 + a];
                xc[k][a] = rgb ? rgb[ii[k] * 3 + a] : 0.0;
                xq[k][a] = nrm ? nrm[ii[k] * 3 + a] : 0.0;
            }
#pragma unroll
        for (int k = 0; k < VB; ++k) {
            if (j0 + k >= end) break;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[a] += xp[k][a];
                if (rgb) c[a] += xc[k][a];
                if (nrm) q[a] += xq[k][a];
            }
        }
    }
    const double cnt = (double)(end - beg);
    const int64_t o = out_row ? (int64_t)out_row[s] : s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        oxyz[o * 3 + a] = p[a] / cnt;
        if (rgb) orgb[o * 3 + a] = c[a] / cnt;
        if (nrm) onrm[o * 3 + a] = q[a] / cnt;
    }
    if (okeys) {
        // recover the integer key of this voxel from its first point (same formula as k_voxel_keys)
        const int64_t i = sidx[beg];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double vmin = ordered_to_dbl(b->mn[a]) - vs * 0.5;
            okeys[o * 3 + a] = (int)floor((xyz[i * 3 + a] - vmin) / vs);
        }
    }
}

}  // namespace
}  // namespace ot
