// voxel.hip — PointCloud::VoxelDownSample on MI355X (check_one_frame.py:28).
//
//   1. bounds      : per-axis min/max with order-preserving u64 atomics (exact, order independent)
//   2. keys        : key = floor((p - (min - vs/2)) / vs) per axis in float64, packed x-major into u64 with
//                    per-axis bit widths from the extent (device-side, no host round trip)
//   3. sort        : stable LSD radix sort of (key, point index)  => equal keys keep input-index order
//   4. heads       : stable compaction of segment starts
//   5. reduce      : one lane per voxel sums its points in index order and divides by the count — the same
//                    float64 operation sequence as Open3D's AccumulatedPoint, so averages are bit-exact.
// Output voxels are in key order (Open3D: unordered_map order; parity compares sorted sets).
#include "voxel_keys.h"

#include "sort.h"

using namespace ot;

extern "C" ot_status ot_voxel_down_sample(const double* xyz, const double* rgb, const double* normals, int64_t n,
                                          double voxel_size, double* out_xyz, double* out_rgb, double* out_normals,
                                          int32_t* out_keys, int64_t* n_out_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (!n_out_host) return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] n_out is NULL");
    if (!(voxel_size > 0.0)) return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] voxel_size <= 0.");
    *n_out_host = 0;
    if (n <= 0) return OT_OK;
    if (!xyz || !out_xyz || (rgb && !out_rgb) || (normals && !out_normals))
        return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] invalid buffers");
    if (n > 0x7FFFFFFF) return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] too many points");
    const size_t un = (size_t)n;
    auto [b, kin, kout, vin, vout, heads] =
        carve(scratch_of(Slot::VOXEL_WS), Arr<Bounds>{1}, Arr<unsigned long long>{un}, Arr<unsigned long long>{un},
              Arr<unsigned>{un}, Arr<unsigned>{un}, Arr<int>{un});
    if (!b) return fail(OT_ERR_HIP, "scratch allocation failed");
    unsigned long long* part = (unsigned long long*)scratch(sizeof(unsigned long long) * BOUNDS_BLOCKS * 6, Slot::VOXEL_BOUNDS_PARTIALS);
    if (!part) return fail(OT_ERR_HIP, "scratch allocation failed");
    launch_bounds(xyz, n, b, part, stream);
    // key width on the host (same float64 formula as k_voxel_keys) so the radix sort runs only the passes the
    // packed key needs
    Bounds hb;
    OT_HIP_TRY(hipMemcpyAsync(&hb, b, sizeof(Bounds), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    const int end_bit = voxel_key_end_bit(hb, voxel_size);
    hipLaunchKernelGGL(k_voxel_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xyz, n, voxel_size, b,
                       kin, vin);
    OT_LAUNCH_CHECK();
    ot_status st = sort_pairs_u64_u32(kin, kout, vin, vout, (size_t)n, end_bit, stream, Slot::SORT_TMP);
    if (st != OT_OK) return st;
    int64_t K = 0;
    st = compact(n, SegHeadPred{kout}, SegHeadEmit{heads}, stream, &K, Slot::VOXEL_HEADS);  // synchronises
    if (st != OT_OK) return st;
    int err = 0;
    OT_HIP_TRY(hipMemcpyAsync(&err, &b->err, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (err == 1) return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] voxel_size is too small.");
    if (err == 2) return fail(OT_ERR_INVALID_ARGUMENT, "[VoxelDownSample] voxel grid exceeds 64-bit key packing");
    hipLaunchKernelGGL(k_voxel_reduce, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, xyz, rgb, normals,
                       vout, kout, heads, K, n, b, voxel_size, out_xyz, out_rgb, out_normals, out_keys,
                       (const int*)nullptr);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n_out_host = K;
    return OT_OK;
}
