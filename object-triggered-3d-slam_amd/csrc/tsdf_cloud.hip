// tsdf_cloud.hip — ScalableTSDFVolume::ExtractPointCloud and ::ExtractVoxelPointCloud on MI355X (DESIGN.md §4 A.9,
// A.10).
//
// Canonical output order (Open3D's follows unordered_map iteration): units in key order (export_units' order), voxel
// x*256 + y*16 + z, and for the zero-crossing cloud axis 0, 1, 2 -- inside a unit Open3D's own loop order.
// Pipeline (one 256-lane workgroup per unit, units in key order):
//   k_cloud_count   : the unit's tsdf and the low faces of its +x / +y / +z neighbours as one 17^3 float tile in LDS,
//                     an unusable voxel (weight == 0 or tsdf outside [-0.98, 0.98)) stored as NaN, so the edge test
//                     f0 * f1 < 0 (a float32 product, as Open3D's) is false for it; per-unit counts of both clouds
//   k_mc_scan2      : both counts' exclusive scans, totals mailed to the host (unit_walk.h)
//   k_cloud_surface : the tile again; lane (x, y) lists its column's cut edges in LDS in output order (one block scan,
//                     LIST_CAP points at a time); then one lane per listed point: position, colour, and the
//                     normal's 6 trilinear samples -- 48 tsdf gathers through the unit's 27-neighbourhood table
//                     (every combination of -1 / 0 / +1 per axis)
//   k_cloud_voxel   : usable voxels, one block scan, centre + (tsdf + 1) / 2 grey
// Every operation is a correctly rounded IEEE operation in the order A.9 / A.10 fix (no contraction), so the clouds
// equal tests/tsdf_cloud_ref.py bit for bit.  Nothing here writes the volume or its marching-cubes structure.
#include <cstring>

#include "tsdf.h"
#include "unit_walk.h"

namespace ot {

constexpr int CT17 = 17;
constexpr int CTILE = CT17 * CT17 * CT17;
constexpr int LIST_CAP = 2048;  // points of a unit listed in LDS at a time (k_cloud_surface)

struct CloudDev {
    const unsigned* sorted_ids;  // rank -> id
    long long* cnt_s;            // [rank] zero-crossing points of the unit
    long long* cnt_v;            // [rank] usable voxels of the unit
    long long* base_s;           // [rank] exclusive scans of the two
    long long* base_v;
};

static void cloud_layout(char* ws, int64_t U, CloudDev& m) {
    const size_t n = ((size_t)U * sizeof(long long) + 255) & ~(size_t)255;
    m.cnt_s = (long long*)ws;
    m.cnt_v = (long long*)(ws + n);
    m.base_s = (long long*)(ws + 2 * n);
    m.base_v = (long long*)(ws + 3 * n);
}
static size_t cloud_ws_bytes(int64_t U) { return 4 * (((size_t)U * sizeof(long long) + 255) & ~(size_t)255); }

__device__ inline bool voxel_usable(float f, float w) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// the unit's 27-neighbourhood: s_nbr[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)] = id of unit key + (dx, dy, dz) or -1
__device__ inline void load_nbr27(const TsdfDev& d, int id, int t, int* s_nbr) {
    if (t < 27) {
        const int dx = t / 9 - 1, dy = (t / 3) % 3 - 1, dz = t % 3 - 1;
        s_nbr[t] = t == 13 ? id
                           : find_unit(d, d.unit_keys[id * 3] + dx, d.unit_keys[id * 3 + 1] + dy,
                                       d.unit_keys[id * 3 + 2] + dz);
    }
}
// id of unit key + (dx, dy, dz): the table inside the 27-neighbourhood, a hash probe outside it (not reached by A.9's
// geometry; kept so that no rounding can index the table out of range)
__device__ inline int nbr_unit(const TsdfDev& d, const int* s_nbr, const int key[3], int dx, int dy, int dz) {
    if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1)
        return s_nbr[(dx + 1) * 9 + (dy + 1) * 3 + dz + 1];
    return find_unit(d, key[0] + dx, key[1] + dy, key[2] + dz);
}

// The 17^3 tile sT[(x * 17 + y) * 17 + z]: the unit's voxels and the faces x == 16, y == 16, z == 16 (the low faces of
// the +x / +y / +z neighbours; the tile's edges and corner are neither written nor read).  tsdf where the voxel is
// usable, NaN elsewhere and for a missing neighbour.  Lane t stages the y-row (z = t >> 4, x = t & 15): 16 contiguous
// floats of each plane, and one voxel of each face.
__device__ inline void stage_tile(const TsdfDev& d, int id, int t, const int* s_nbr, float* sT) {
    const float nan = __builtin_nanf("");
    const int a = t >> 4, b = t & 15;
    const float* own = unit_base(d, id);
    const float4* tp = reinterpret_cast<const float4*>(own) + t * 4;
    const float4* wp = reinterpret_cast<const float4*>(own + UNIT_VOX) + t * 4;
    float4 tv[4], wv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tv[k] = tp[k];
        wv[k] = wp[k];
    }
    float fy = 0.0f, wy = 0.0f, fx = 0.0f, wx = 0.0f, fz = 0.0f, wz = 0.0f;
    const int nx = s_nbr[22], ny = s_nbr[16], nz = s_nbr[14];
    if (ny >= 0) {
        fy = unit_base(d, ny)[a * 256 + b * 16];
        wy = unit_base(d, ny)[UNIT_VOX + a * 256 + b * 16];
    }
    if (nx >= 0) {
        fx = unit_base(d, nx)[a * 256 + b];
        wx = unit_base(d, nx)[UNIT_VOX + a * 256 + b];
    }
    if (nz >= 0) {
        fz = unit_base(d, nz)[a * 16 + b];
        wz = unit_base(d, nz)[UNIT_VOX + a * 16 + b];
    }
    const float f16[16] = {tv[0].x, tv[0].y, tv[0].z, tv[0].w, tv[1].x, tv[1].y, tv[1].z, tv[1].w,
                           tv[2].x, tv[2].y, tv[2].z, tv[2].w, tv[3].x, tv[3].y, tv[3].z, tv[3].w};
    const float w16[16] = {wv[0].x, wv[0].y, wv[0].z, wv[0].w, wv[1].x, wv[1].y, wv[1].z, wv[1].w,
                           wv[2].x, wv[2].y, wv[2].z, wv[2].w, wv[3].x, wv[3].y, wv[3].z, wv[3].w};
#pragma unroll
    for (int y = 0; y < 16; ++y) sT[(b * CT17 + y) * CT17 + a] = voxel_usable(f16[y], w16[y]) ? f16[y] : nan;
    sT[(b * CT17 + 16) * CT17 + a] = voxel_usable(fy, wy) ? fy : nan;
    sT[(16 * CT17 + b) * CT17 + a] = voxel_usable(fx, wx) ? fx : nan;
    sT[(a * CT17 + b) * CT17 + 16] = voxel_usable(fz, wz) ? fz : nan;
}

// cut edges of voxel (x, y, z) as a 3-bit mask (bit a: the edge along axis a emits a point); usable: the voxel is
__device__ inline int voxel_edges(const float* sT, int x, int y, int z, bool& usable) {
    const int c = (x * CT17 + y) * CT17 + z;
    const float f0 = sT[c];
    usable = f0 == f0;
    // a NaN (unusable voxel on either end) and signed zeros compare false
    return (f0 * sT[c + CT17 * CT17] < 0.0f ? 1 : 0) | (f0 * sT[c + CT17] < 0.0f ? 2 : 0) |
           (f0 * sT[c + 1] < 0.0f ? 4 : 0);
}

__global__ __launch_bounds__(256) void k_cloud_count(TsdfDev d, CloudDev m) {
    __shared__ float sT[CTILE];
    __shared__ int s_nbr[27];
    __shared__ int wsum[4][2];
    const int r = blockIdx.x, t = threadIdx.x;
    const int id = (int)m.sorted_ids[r];
    load_nbr27(d, id, t, s_nbr);
    __syncthreads();
    stage_tile(d, id, t, s_nbr, sT);
    __syncthreads();
    const int x = t >> 4, y = t & 15;
    int ns = 0, nv = 0;
#pragma unroll
    for (int z = 0; z < UNIT_RES; ++z) {
        bool us;
        ns += __popc((unsigned)voxel_edges(sT, x, y, z, us));
        nv += us ? 1 : 0;
    }
    ns = wave_sum(ns);
    nv = wave_sum(nv);
    if (lane_id() == 0) {
        wsum[t >> 6][0] = ns;
        wsum[t >> 6][1] = nv;
    }
    __syncthreads();
    if (t == 0) {
        m.cnt_s[r] = (long long)(wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0]);
        m.cnt_v[r] = (long long)(wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1]);
    }
}

// GetTSDFAt(q) (A.9): trilinear interpolation of the stored tsdf (weights ignored) in float64, in Open3D's association
__device__ inline double tsdf_at(const TsdfDev& d, const int* s_nbr, const int key[3], double vl, double UL,
                                 double half, const double q[3]) {
    int du[3], i[3];
    double r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ql = q[a] - half;
        const double uf = floor(ql / UL);
        // no unit lies outside the key range (a NaN fails the test too)
        if (!(uf >= -(double)KEY_BIAS && uf < (double)KEY_BIAS)) return 0.0;
        const double g = (ql - uf * UL) / vl;
        int ii = (int)floor(g);
        ii = ii < 0 ? 0 : (ii > UNIT_RES - 1 ? UNIT_RES - 1 : ii);
        i[a] = ii;
        r[a] = g - (double)ii;
        du[a] = (int)uf - key[a];  // both inside the key range: no overflow
    }
    if (nbr_unit(d, s_nbr, key, du[0], du[1], du[2]) < 0) return 0.0;
    // corners in A.9's order: shift = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)
    constexpr int sh[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
    double f[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cx = i[0] + sh[c][0], cy = i[1] + sh[c][1], cz = i[2] + sh[c][2];  // in [0, 16]
        const int nid = nbr_unit(d, s_nbr, key, du[0] + (cx >> 4), du[1] + (cy >> 4), du[2] + (cz >> 4));
        f[c] = nid >= 0 ? (double)unit_base(d, nid)[(cz & 15) * 256 + (cx & 15) * 16 + (cy & 15)] : 0.0;
    }
    const double r0 = r[0], r1 = r[1], r2 = r[2];
    return (1 - r0) * ((1 - r1) * ((1 - r2) * f[0] + r2 * f[4]) + r1 * ((1 - r2) * f[3] + r2 * f[7])) +
           r0 * ((1 - r1) * ((1 - r2) * f[1] + r2 * f[5]) + r1 * ((1 - r2) * f[2] + r2 * f[6]));
}

// one listed point (code = local voxel * 3 + axis) into row `row`: position, colour (C != nullptr) and normal
template <typename CT>
__device__ __forceinline__ void cloud_point(const TsdfDev& d, const int* s_nbr, const float* sT, int id,
                                            const int key[3], double vl, int code, long long row, double* __restrict__ P,
                                            double* __restrict__ N, double* __restrict__ C) {
    const double half = vl * 0.5, UL = vl * (double)UNIT_RES, gap = 0.99 * vl;
    const int local = code / 3, a = code % 3;
    const int v0[3] = {local >> 8, (local >> 4) & 15, local & 15};
    const int v1[3] = {v0[0] + (a == 0), v0[1] + (a == 1), v0[2] + (a == 2)};
    const float f0 = sT[(v0[0] * CT17 + v0[1]) * CT17 + v0[2]];
    const float f1 = sT[(v1[0] * CT17 + v1[1]) * CT17 + v1[2]];
    const float r0 = fabsf(f0), r1 = fabsf(f1), rs = r0 + r1;
    double p[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) p[b] = (half + vl * (double)v0[b]) + (double)key[b] * UL;
    {
        const double pa0 = a == 0 ? p[0] : (a == 1 ? p[1] : p[2]);
        const double pa1 = pa0 + vl;
        const double pa = (pa0 * (double)r1 + pa1 * (double)r0) / (double)rs;
        if (a == 0) p[0] = pa;
        else if (a == 1) p[1] = pa;
        else p[2] = pa;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) P[row * 3 + b] = p[b];
    if (C) {
        const int nid = s_nbr[((v1[0] >> 4) + 1) * 9 + ((v1[1] >> 4) + 1) * 3 + (v1[2] >> 4) + 1];
        const int vi0 = v0[2] * 256 + v0[0] * 16 + v0[1];
        const int vi1 = (v1[2] & 15) * 256 + (v1[0] & 15) * 16 + (v1[1] & 15);
        const CT* cb0 = color_base<CT>(d, id);
        // (the neighbour holds a usable voxel, so it exists; never read through a missing id)
        const CT* cb1 = nid >= 0 ? color_base<CT>(d, nid) : cb0;
        const int vj = nid >= 0 ? vi1 : vi0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float c0 = (float)cb0[b * UNIT_VOX + vi0], c1 = (float)cb1[b * UNIT_VOX + vj];
            C[row * 3 + b] = (double)(((c0 * r1 + c1 * r0) / rs) / 255.0f);
        }
    }
    // GetNormalAt(p): central differences of the interpolated tsdf at +-0.99 voxel, Eigen's normalized()
    double n[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        double q[3] = {p[0], p[1], p[2]};
        q[b] = p[b] + gap;
        const double tp = tsdf_at(d, s_nbr, key, vl, UL, half, q);
        q[b] = p[b] - gap;
        const double tm = tsdf_at(d, s_nbr, key, vl, UL, half, q);
        n[b] = tp - tm;
    }
    const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (s > 0.0) {
        const double sq = sqrt(s);
        n[0] /= sq;
        n[1] /= sq;
        n[2] /= sq;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) N[row * 3 + b] = n[b];
}

// CT: the volume's colour planes (float / double); C == nullptr: no colours (NoColor volumes, or not asked for)
// 5 waves per SIMD (96 VGPRs, no scratch; 6 would spill): a point is one lane's chain of dependent gathers, and the
// 24 KB of LDS would allow six workgroups per CU
template <typename CT>
__global__ __launch_bounds__(256, 5) void k_cloud_surface(TsdfDev d, CloudDev m, double vl, double* __restrict__ P,
                                                       double* __restrict__ N, double* __restrict__ C) {
    __shared__ float sT[CTILE];
    __shared__ unsigned short s_list[LIST_CAP];  // listed points: local voxel * 3 + axis, in output order
    __shared__ int s_nbr[27];
    const int r = blockIdx.x, t = threadIdx.x;
    const int id = (int)m.sorted_ids[r];
    if (m.cnt_s[r] == 0) return;  // block-uniform
    load_nbr27(d, id, t, s_nbr);
    __syncthreads();
    stage_tile(d, id, t, s_nbr, sT);
    __syncthreads();
    const int x = t >> 4, y = t & 15;
    unsigned em[2] = {0u, 0u};  // the column's edge masks, 3 bits per z
    int cnt = 0;
#pragma unroll
    for (int z = 0; z < UNIT_RES; ++z) {
        bool us;
        const int e = voxel_edges(sT, x, y, z, us);
        em[z >> 3] |= (unsigned)e << ((z & 7) * 3);
        cnt += __popc((unsigned)e);
    }
    int total;
    const int first = block_excl_scan_n<256>(cnt, total);
    const long long base = m.base_s[r];
    const int key[3] = {d.unit_keys[id * 3], d.unit_keys[id * 3 + 1], d.unit_keys[id * 3 + 2]};
    // the list in chunks of LIST_CAP points (a unit of a scan holds a few hundred: one chunk; `total` is block-uniform)
    for (int lo = 0; lo < total; lo += LIST_CAP) {
        if (lo) __syncthreads();  // the previous chunk has been read
        if (first < lo + LIST_CAP && first + cnt > lo) {
            int slot = first - lo;
#pragma unroll
            for (int z = 0; z < UNIT_RES; ++z) {
                const unsigned e = (em[z >> 3] >> ((z & 7) * 3)) & 7u;
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    if ((e >> a) & 1u) {
                        if (slot >= 0 && slot < LIST_CAP) s_list[slot] = (unsigned short)((t * 16 + z) * 3 + a);
                        ++slot;
                    }
            }
        }
        __syncthreads();
        const int chunk = total - lo < LIST_CAP ? total - lo : LIST_CAP;
        for (int i = t; i < chunk; i += 256)
            cloud_point<CT>(d, s_nbr, sT, id, key, vl, (int)s_list[i], base + lo + i, P, N, C);
    }
}

// ExtractVoxelPointCloud: lane (x, y) owns the column's 16 voxels, which are consecutive in output order
__global__ __launch_bounds__(256) void k_cloud_voxel(TsdfDev d, CloudDev m, double vl, double* __restrict__ P,
                                                     double* __restrict__ C) {
    const int r = blockIdx.x, t = threadIdx.x;
    const int id = (int)m.sorted_ids[r];
    if (m.cnt_v[r] == 0) return;  // block-uniform
    const float* base = unit_base(d, id);
    float f[UNIT_RES];
    unsigned us = 0u;
    // record index z*256 + x*16 + y = z*256 + t: a coalesced row per z
#pragma unroll
    for (int z = 0; z < UNIT_RES; ++z) {
        f[z] = base[z * 256 + t];
        us |= voxel_usable(f[z], base[UNIT_VOX + z * 256 + t]) ? 1u << z : 0u;
    }
    int total;
    long long row = m.base_v[r] + block_excl_scan_n<256>(__popc(us), total);
    const int x = t >> 4, y = t & 15;
    const double half = vl * 0.5, UL = vl * (double)UNIT_RES;
    const double px = (half + vl * (double)x) + (double)d.unit_keys[id * 3] * UL;
    const double py = (half + vl * (double)y) + (double)d.unit_keys[id * 3 + 1] * UL;
    const double oz = (double)d.unit_keys[id * 3 + 2] * UL;
#pragma unroll
    for (int z = 0; z < UNIT_RES; ++z) {
        if (!((us >> z) & 1u)) continue;
        P[row * 3 + 0] = px;
        P[row * 3 + 1] = py;
        P[row * 3 + 2] = (half + vl * (double)z) + oz;
        const double c = ((double)f[z] + 1.0) * 0.5;
        C[row * 3 + 0] = c;
        C[row * 3 + 1] = c;
        C[row * 3 + 2] = c;
        ++row;
    }
}

// Both clouds' per-unit counts, scans and totals (one read-back).  who: the Open3D call's name for the messages.
static ot_status cloud_count(ot_tsdf* vol, hipStream_t stream, const char* who) {
    CloudBuffers& cb = vol->cloud;
    cb.valid = false;
    cb.n_surface = cb.n_voxel = 0;
    if (vol->dev.shard_world > 1)
        return fail(OT_ERR_INVALID_ARGUMENT,
                    std::string("[") + who + "] not available on a spatially sharded volume (the normals read units of "
                    "other shards): extract from the volume distributed.assemble_sharded_volume returns");
    int64_t U = 0;
    ot_status st = tsdf_sorted_units(vol, stream, &U);  // integrates the queued frames first
    if (st != OT_OK) return st;
    cb.valid = false;
    cb.units = U;
    if (U == 0) {
        cb.valid = true;
        return OT_OK;
    }
    const size_t bytes = cloud_ws_bytes(U);
    if (cb.ws_bytes < bytes) {
        if (cb.ws) {
            OT_HIP_TRY(hipStreamSynchronize(stream));  // an earlier emission may still read the bases
            OT_HIP_TRY(hipFree(cb.ws));
            cb.ws = nullptr;
            cb.ws_bytes = 0;
        }
        const size_t nb = cloud_ws_bytes(U + U / 4);
        OT_HIP_TRY(hipMalloc(&cb.ws, nb));
        cb.ws_bytes = nb;
        note_alloc();
    }
    CloudDev m;
    m.sorted_ids = vol->sorted_ids;
    cloud_layout((char*)cb.ws, U, m);
    hipLaunchKernelGGL(k_cloud_count, dim3((unsigned)U), dim3(256), 0, stream, vol->dev, m);
    OT_LAUNCH_CHECK();
    // the scans mail the two totals (hmail words 0..3), as marching cubes' do
    const unsigned seq = ++vol->mc_seq;
    hipLaunchKernelGGL(k_mc_scan2, dim3(2), dim3(1024), 0, stream, (const long long*)m.cnt_s, m.base_s,
                       (const long long*)m.cnt_v, m.base_v, (int)U, (long long*)vol->hmail, vol->hmail + MAIL_SEQ_MC,
                       seq);
    OT_LAUNCH_CHECK();
    st = mail_wait(vol->hmail + MAIL_SEQ_MC, seq, stream);
    if (st == OT_OK) st = mail_wait(vol->hmail + MAIL_SEQ_MC + 1, seq, stream);
    if (st != OT_OK) return st;
    long long totals[2];
    std::memcpy(totals, vol->hmail, sizeof(totals));
    cb.n_surface = totals[0];
    cb.n_voxel = totals[1];
    cb.valid = true;
    return OT_OK;
}

static ot_status cloud_ready(const ot_tsdf* vol, const char* who) {
    if (!vol) return fail(OT_ERR_INVALID_ARGUMENT, std::string("[") + who + "] volume is NULL");
    if (!vol->cloud.valid)
        return fail(OT_ERR_INVALID_ARGUMENT, std::string("[") + who + "] the volume changed since the count");
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_tsdf_extract_point_cloud_count(ot_tsdf* vol, int64_t* n_points, void* stream) {
    if (!vol || !n_points) return fail(OT_ERR_INVALID_ARGUMENT, "[ExtractPointCloud] invalid arguments");
    *n_points = 0;
    ot_status st = cloud_count(vol, S(stream), "ExtractPointCloud");
    if (st == OT_OK) *n_points = vol->cloud.n_surface;
    return st;
}

ot_status ot_tsdf_emit_point_cloud(ot_tsdf* vol, double* points, double* normals, double* colors, void* stream) {
    ot_status st = cloud_ready(vol, "ExtractPointCloud");
    if (st != OT_OK) return st;
    const CloudBuffers& cb = vol->cloud;
    if (cb.n_surface == 0) return OT_OK;
    if (!points || !normals) return fail(OT_ERR_INVALID_ARGUMENT, "[ExtractPointCloud] invalid arguments");
    CloudDev m;
    m.sorted_ids = vol->sorted_ids;
    cloud_layout((char*)cb.ws, cb.units, m);
    double* c = vol->color_type == OT_COLOR_RGB8 ? colors : nullptr;
    if (vol->color64)
        hipLaunchKernelGGL(k_cloud_surface<double>, dim3((unsigned)cb.units), dim3(256), 0, S(stream), vol->dev, m,
                           vol->voxel_length, points, normals, c);
    else
        hipLaunchKernelGGL(k_cloud_surface<float>, dim3((unsigned)cb.units), dim3(256), 0, S(stream), vol->dev, m,
                           vol->voxel_length, points, normals, c);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

ot_status ot_tsdf_extract_voxel_point_cloud_count(ot_tsdf* vol, int64_t* n_points, void* stream) {
    if (!vol || !n_points) return fail(OT_ERR_INVALID_ARGUMENT, "[ExtractVoxelPointCloud] invalid arguments");
    *n_points = 0;
    ot_status st = cloud_count(vol, S(stream), "ExtractVoxelPointCloud");
    if (st == OT_OK) *n_points = vol->cloud.n_voxel;
    return st;
}

ot_status ot_tsdf_emit_voxel_point_cloud(ot_tsdf* vol, double* points, double* colors, void* stream) {
    ot_status st = cloud_ready(vol, "ExtractVoxelPointCloud");
    if (st != OT_OK) return st;
    const CloudBuffers& cb = vol->cloud;
    if (cb.n_voxel == 0) return OT_OK;
    if (!points || !colors) return fail(OT_ERR_INVALID_ARGUMENT, "[ExtractVoxelPointCloud] invalid arguments");
    CloudDev m;
    m.sorted_ids = vol->sorted_ids;
    cloud_layout((char*)cb.ws, cb.units, m);
    hipLaunchKernelGGL(k_cloud_voxel, dim3((unsigned)cb.units), dim3(256), 0, S(stream), vol->dev, m, vol->voxel_length,
                       points, colors);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // extern "C"
