/*
 * otslam.h — C ABI of the MI355X-native RGB-D reconstruction / voxel-filter path.
 *
 * This is the drop-in boundary.  The reference (TakiRyo/object-triggered-3D-SLAM) has no FFI of its own:
 * its scripts call the Open3D Python API directly.  Every entry point below replaces one
 * Open3D call made on the hot path; the reference call site it stands behind is cited per function.
 * The Python facade (object-triggered-3d-slam_amd/) binds these with ctypes and keeps Open3D's names,
 * keyword arguments, defaults and RuntimeError behaviour.
 *
 * Conventions
 *   - All bulk arrays are DEVICE pointers (HBM of the device current for the calling thread) unless the
 *     parameter name ends in `_host`.  Small parameter blocks (intrinsics, 4x4 matrices) are host memory.
 *   - `stream` is a hipStream_t passed as void*; NULL = the null stream.  Functions that must return a
 *     size to the host (n_points, n_kept, ...) synchronise that stream before returning.
 *   - Matrices are row-major double[16] (numpy's default layout for a 4x4 float64 array).
 *   - Return value: OT_OK (0) or an error code; ot_last_error() returns a thread-local message in the
 *     Open3D style ("[ScalableTSDFVolume::Integrate] Unsupported image format.").
 *   - Point clouds are SoA-free AoS float64 [n][3] exactly like Open3D's std::vector<Eigen::Vector3d>.
 */
#ifndef OTSLAM_H
#define OTSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int ot_status;
#define OT_OK 0
#define OT_ERR_INVALID_ARGUMENT 1
#define OT_ERR_UNSUPPORTED_FORMAT 2
#define OT_ERR_CAPACITY 3
#define OT_ERR_HIP 4

/* TSDFVolumeColorType (open3d.pipelines.integration.TSDFVolumeColorType) */
#define OT_COLOR_NONE 0
#define OT_COLOR_RGB8 1

/* camera.PinholeCameraIntrinsic(width, height, fx, fy, cx, cy) — reconstruct_rgbd_filter.py:26-29 */
typedef struct ot_intrinsics {
    int32_t width;
    int32_t height;
    double fx, fy, cx, cy;
} ot_intrinsics;

const char* ot_last_error(void);
const char* ot_version(void);
int32_t ot_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * Images
 * ------------------------------------------------------------------------------------------------- */

/* geometry.RGBDImage.create_from_color_and_depth(color, depth, depth_scale, depth_trunc,
 *     convert_rgb_to_intensity=False) — depth part (Open3D Image::ConvertDepthToFloatImage).
 * Replaces reconstruct_rgbd_filter.py:98-103 and check_one_frame.py:22-25.
 * out[i] = (float)in[i] / (float)depth_scale; out[i] = 0 if out[i] >= depth_trunc. */
ot_status ot_depth_to_float(const uint16_t* depth_u16, float* depth_f32, int64_t n_pixels,
                            double depth_scale, double depth_trunc, void* stream);

/* Open3D Image::CreateDepthToCameraDistanceMultiplierFloatImage (called inside
 * ScalableTSDFVolume::Integrate, reconstruct_rgbd_filter.py:105).  out: float [height][width]. */
ot_status ot_depth_multiplier(const ot_intrinsics* intrinsic, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Point clouds
 * ------------------------------------------------------------------------------------------------- */

/* geometry.PointCloud.create_from_rgbd_image(rgbd, intrinsic, extrinsic)   (color != NULL, RGB8)
 * geometry.PointCloud.create_from_depth_image(depth, intrinsic, extrinsic, stride) (color == NULL)
 * Replaces check_one_frame.py:27.  Valid pixels (d > 0) in row-major order; xyz = inverse(extrinsic) *
 * ((j-cx)*z/fx, (i-cy)*z/fy, z, 1) in float64; rgb = color/255.  out_xyz/out_rgb: [capacity][3].
 * capacity must be >= ceil(h/stride)*ceil(w/stride).  *n_points_host receives P. */
ot_status ot_unproject(const float* depth, const uint8_t* color, const ot_intrinsics* intrinsic,
                       const double extrinsic[16], int32_t stride, double* out_xyz, double* out_rgb,
                       int64_t capacity, int64_t* n_points_host, void* stream);

/* geometry.PointCloud.voxel_down_sample(voxel_size) — check_one_frame.py:28.
 * Voxels are emitted sorted by (kx, ky, kz) lexicographically (Open3D emits hash order; parity compares
 * the sorted set).  Averages are sum/count in float64 with the sum taken in input-index order.
 * rgb / normals may be NULL (then their outputs are ignored).  out_keys (nullable): int32 [K][3].
 * Output buffers must hold n rows. */
ot_status ot_voxel_down_sample(const double* xyz, const double* rgb, const double* normals, int64_t n,
                               double voxel_size, double* out_xyz, double* out_rgb, double* out_normals,
                               int32_t* out_keys, int64_t* n_out_host, void* stream);

/* geometry.PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio) — north_star (not called by
 * the reference scripts; Open3D API contract).  Writes the kept indices
 * (ascending, int64) and, if out_avg_dist != NULL, the per-point mean kNN distance (-1 when none). */
ot_status ot_remove_statistical_outlier(const double* xyz, int64_t n, int32_t nb_neighbors,
                                        double std_ratio, int64_t* out_indices, double* out_avg_dist,
                                        int64_t* n_kept_host, void* stream);

/* geometry.PointCloud.remove_radius_outlier(nb_points, radius) — Appendix A.7.  Keeps i when
 * |{j : |pj - pi|^2 < radius^2}| > nb_points (self included).  Writes kept indices ascending. */
ot_status ot_remove_radius_outlier(const double* xyz, int64_t n, int32_t nb_points, double radius,
                                   int64_t* out_indices, int64_t* n_kept_host, void* stream);

/* geometry.PointCloud.cluster_dbscan(eps, min_points) — Open3D's PointCloud::ClusterDBSCAN ("DBSCAN").
 * With d2(i, j) = ((dx dx) + dy dy) + dz dz in float64 (ROR's test): point i is a core point when
 * |{j : d2(i, j) < eps^2}| >= min_points (i itself counts, so min_points 0 and 1 make every point core); clusters are
 * the connected components of the core points under d2 < eps^2, numbered 0 .. C-1 by ascending smallest point index
 * among their core members; a non-core point takes the smallest label among the core points within eps of it, and
 * -1 (noise) when there is none.  These are the labels of Open3D's index-order loop.  out_labels: device int32 [n] in
 * input order; *n_clusters_host (nullable) receives C.  eps must be finite and > 0 and min_points >= 0
 * (OT_ERR_INVALID_ARGUMENT, checked before any device work); n == 0 returns at once. */
ot_status ot_cluster_dbscan(const double* xyz, int64_t n, double eps, int32_t min_points,
                            int32_t* out_labels /* device [n], input order */,
                            int32_t* n_clusters_host, void* stream);

/* geometry.PointCloud.segment_plane(distance_threshold, ransac_n, num_iterations, probability, seed) — Open3D's
 * PointCloud::SegmentPlane with a seeded sampler ("Plane segmentation", holds the whole definition).
 * Iteration it keeps the first ransac_n distinct indices among z(seed, (it << 32) + t) mod n, t = 0, 1, ... (z: the
 * counter RNG of the mesh sampler), fits their plane (3 points: the triangle's plane; more: GetPlaneFromPoints), and
 * counts the points with |((a x + b y) + c z) + d| < distance_threshold (strict).  Open3D's serial loop is replayed on
 * those counts: a zero plane is skipped without counting, the best candidate is the one of highest count and, among
 * equal counts, smallest inlier_rmse = (serial sum of the inlier distances) / sqrt(k), the earliest among equal ones;
 * the loop stops once the iterations counted exceed trunc(log(1 - probability) / log(1 - fitness^ransac_n)).
 * inliers: the best plane's inlier indices ascending (device int64, capacity n); plane_host: GetPlaneFromPoints over
 * them (a, b, c, d; the zero plane when there are none); *evaluated_host (nullable): iterations counted.  All float64,
 * no contraction; two calls give the same bits.  Errors (OT_ERR_INVALID_ARGUMENT, before any device work, in this
 * order): probability outside (0, 1], ransac_n < 3, n < ransac_n; ransac_n > 32 is not supported by this build. */
ot_status ot_segment_plane(const double* xyz, int64_t n, double distance_threshold, int32_t ransac_n,
                           int32_t num_iterations, double probability, uint64_t seed, double plane_host[4],
                           int64_t* inliers /* device int64, capacity n */, int64_t* n_inliers_host,
                           int32_t* evaluated_host /* iterations counted */, void* stream);

/* geometry.PointCloud.estimate_covariances(search_param) — Open3D's EstimatePerPointCovariances (DESIGN.md §4,
 * "normals").  Neighbours of point i: every point j of the cloud (i included) ordered ascending by (d2, j) with
 * d2 = ((dx dx) + dy dy) + dz dz in float64; the first min(knn, n) of them, and with radius > 0 (hybrid search) only
 * those of these with d2 < radius^2 (strict).  radius <= 0: pure KNN.  With m neighbours, m < 3: the identity;
 * otherwise the nine sums x, y, z, xx, xy, xz, yy, yz, zz over the neighbours in that order (each product rounded,
 * then added), each divided by (double)m, and C00 = s3 - s0 s0, C01 = s4 - s0 s1, ... (not centred first).
 * cov_out: device float64 [n][3][3] in input order.  knn must lie in 1..64 and radius must not be NaN
 * (OT_ERR_INVALID_ARGUMENT, checked before any device work); n == 0 returns at once. */
ot_status ot_estimate_covariances(const double* xyz, int64_t n, int32_t knn, double radius,
                                  double* cov_out /* device [n][9] */, void* stream);

/* geometry.PointCloud.estimate_normals(search_param, fast_normal_computation=True): the covariances of
 * ot_estimate_covariances, then per point the eigenvector of the smallest eigenvalue by Open3D's FastEigen3x3
 * (the non-iterative symmetric 3x3 solver; DESIGN.md §4 spells out every branch).  A zero result becomes the point's
 * prior normal, or (0, 0, 1) without priors; with priors the result is negated when its dot product with the prior
 * is negative.  prior_normals (nullable): device [n][3], may alias normals_out.  cov_out (nullable): receives the
 * covariances.  Argument rules as ot_estimate_covariances. */
ot_status ot_estimate_normals(const double* xyz, int64_t n, int32_t knn, double radius, const double* prior_normals,
                              double* normals_out /* device [n][3] */, double* cov_out /* device [n][9] or NULL */,
                              void* stream);

/* geometry.PointCloud.orient_normals_to_align_with_direction (mode 0, ref3_host = the direction) and
 * orient_normals_towards_camera_location (mode 1, ref3_host = the camera location; the reference vector of point i is
 * then v = ref - xyz[i]), in place.  A zero normal becomes the reference vector (mode 1: v / |v|, or (0, 0, 1) when v
 * is zero too); any other normal is negated when (nx rx + ny ry) + nz rz < 0.  xyz is read in mode 1 only. */
ot_status ot_orient_normals(double* normals_inout, const double* xyz, int64_t n, int32_t mode,
                            const double ref3_host[3], void* stream);

/* geometry.PointCloud.normalize_normals(), in place: n / sqrt((nx nx + ny ny) + nz nz); a zero normal stays zero. */
ot_status ot_normalize_normals(double* normals_inout, int64_t n, void* stream);

/* Stable compaction `mask = points[:, 2] >= z_min` — reconstruct_rgbd_filter.py:126-132.
 * rgb may be NULL.  Output buffers hold n rows. */
ot_status ot_filter_min_z(const double* xyz, const double* rgb, int64_t n, double z_min,
                          double* out_xyz, double* out_rgb, int64_t* n_out_host, void* stream);

/* Gather rows: out[k] = in[idx[k]] for k < m (PointCloud.select_by_index / SelectByIndex). */
ot_status ot_gather_rows3(const double* in, const int64_t* idx, int64_t m, double* out, void* stream);

/* geometry.PointCloud.compute_point_cloud_distance(target) — eval_cone.py:99,103 (accuracy / completeness).
 * out[i] = sqrt(min_j |src_i - tgt_j|^2) in float64 (exact minimum, nanoflann L2 accumulation order);
 * 0.0 for every point when the target is empty (Open3D: no neighbour found). */
ot_status ot_compute_point_cloud_distance(const double* src, int64_t n, const double* tgt, int64_t m,
                                          double* out, void* stream);

/* geometry.PointCloud.transform(T) — eval_cone.py:96.  T_host: row-major 4x4 on the host.  Per point (Eigen's
 * column-order product, no contraction): x' = ((T00 x + T01 y) + T02 z) + T03 (rows 1..3 alike), then xyz' / w'.
 * normals (nullable, with out_normals) are multiplied by the upper 3x3 block and not renormalised.  out may alias
 * the input. */
ot_status ot_transform_points(const double* xyz, const double* normals, int64_t n, const double T_host[16],
                              double* out_xyz, double* out_normals, void* stream);

/* pipelines.registration.evaluate_registration(source, target, max_correspondence_distance, T) (DESIGN.md §4,
 * "registration"): pcd = T source; per pcd point the nearest target point by exact float64 squared distance
 * ((dx dx + dy dy) + dz dz; equidistant targets: the lowest index), a correspondence iff d2 < r r (strict);
 * fitness = k / n, inlier_rmse = sqrt(sum d2 / k), both 0 when k = 0.  corr (device int32 [n][2], nullable) receives
 * the k (source index, target index) pairs in ascending source index.  Empty source or target, or
 * max_corr_dist <= 0: zeros, no pairs. */
ot_status ot_evaluate_registration(const double* src, int64_t n, const double* tgt, int64_t m, double max_corr_dist,
                                   const double T_host[16], double* fitness_host, double* rmse_host, int32_t* corr,
                                   int64_t* n_corr_host, void* stream);

/* pipelines.registration.registration_icp(source, target, max_correspondence_distance, init,
 * TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))
 * — eval_cone.py:89-97.  Each iteration fits the rigid update of the current correspondences (Eigen::umeyama without
 * scaling), moves the kept cloud by it, re-evaluates, and stops once fitness and inlier_rmse both change by less than
 * their thresholds; the whole loop runs on the device.  Outputs as ot_evaluate_registration for the last evaluation,
 * T_out_host = the accumulated transformation (row-major), iterations_host = fits performed.  Empty source or
 * target: zeros, no pairs, T = init.  max_corr_dist <= 0 fails with "Invalid max_correspondence_distance." */
ot_status ot_registration_icp(const double* src, int64_t n, const double* tgt, int64_t m, double max_corr_dist,
                              const double init_host[16], double relative_fitness, double relative_rmse,
                              int32_t max_iteration, double T_out_host[16], double* fitness_host, double* rmse_host,
                              int32_t* corr, int64_t* n_corr_host, int32_t* iterations_host, void* stream);

/* pipelines.registration.compute_fpfh_feature(input, search_param) ("features"): per point the 33-bin
 * Fast Point Feature Histogram over the neighbour list of ot_estimate_covariances (ascending (d2, index), the first
 * min(knn, n), hybrid: of these the ones with d2 < radius^2; radius == 0: pure KNN).  Entry 0 of a list is skipped as
 * "the query itself".  SPFH: per remaining entry the three Darboux pair features, each binned into 11 bins with
 * weight 100 / (len - 1), added in list order.  FPFH: the neighbours' SPFH rows weighted by 1 / d2 (entries with
 * d2 == 0 skipped), each block of 11 scaled to sum 100, plus the point's own SPFH.  Everything is float64, every
 * operation rounded on its own.  xyz, normals: device [n][3]; fpfh_out: device [n][33], point-major; spfh_out
 * (nullable): device [n][33], receives the SPFH.  knn must lie in 1..128 and radius must not be NaN
 * (OT_ERR_INVALID_ARGUMENT, checked before any device work); n == 0 returns at once. */
ot_status ot_compute_fpfh_feature(const double* xyz, const double* normals, int64_t n, int32_t knn, double radius,
                                  double* fpfh_out /* n x 33, point-major */, double* spfh_out /* optional */,
                                  void* stream);

/* pipelines.registration.correspondences_from_features(source, target, mutual_filter, mutual_consistency_ratio)
 * ("features").  src, tgt: device float64, point-major (one row of dim values per feature column of
 * Open3D's Feature.data).  The match of source row i is the target row with the smallest (d2, index), d2 the
 * sequential sum over j = 0 .. dim-1 of (s_j - t_j) (s_j - t_j).  Without mutual_filter corr_out (device int32
 * [n][2]) receives (i, match(i)) for every i.  With it the targets are matched against the source the same way and
 * only the pairs with match_t(match(i)) == i are kept, in i order; if fewer than
 * mutual_consistency_ratio * (double)n are kept, all n pairs are returned instead and *fell_back_host (nullable) is
 * set to 1 (0 otherwise).  dim must lie in 1..128; n == 0 gives zero pairs; m == 0 with n > 0 is refused. */
ot_status ot_correspondences_from_features(const double* src /* n x dim */, int64_t n, const double* tgt /* m x dim */,
                                           int64_t m, int32_t dim, int32_t mutual_filter, double mutual_consistency_ratio,
                                           int32_t* corr_out /* n x 2 */, int64_t* n_corr_host, int32_t* fell_back_host,
                                           void* stream);

/* The configs[2] filter chain for a batch of frames, device-resident end to end (not an Open3D API: the batch form
 * of the per-frame calls below, results bit-identical to them).  Per frame f of a run:
 *   create_from_color_and_depth(depth_scale, depth_trunc) -> PointCloud.create_from_rgbd_image(intrinsic,
 *   extrinsic_f) -> voxel_down_sample(voxel_size) -> remove_statistical_outlier(nb_neighbors, std_ratio)
 *   -> select_by_index(kept)
 * i.e. check_one_frame.py:22-28 (with a pose) followed by the north_star's statistical filter.  A handle keeps its
 * device buffers between runs (grow-only).  Not thread-safe per handle. */
typedef struct ot_rgbd_filter ot_rgbd_filter;
ot_status ot_rgbd_filter_create(const ot_intrinsics* intrinsic, int32_t max_frames, double depth_scale,
                                double depth_trunc, double voxel_size, int32_t nb_neighbors, double std_ratio,
                                ot_rgbd_filter** out);
ot_status ot_rgbd_filter_destroy(ot_rgbd_filter* filter);
/* depth: uint16 [n_frames][h][w], color: uint8 [n_frames][h][w][3] (device, contiguous); extrinsics_host:
 * double [n_frames][16] row-major.  Synchronises `stream` (the result sizes come back to the host). */
ot_status ot_rgbd_filter_run(ot_rgbd_filter* filter, int32_t n_frames, const uint16_t* depth, const uint8_t* color,
                             const double* extrinsics_host, void* stream);
/* Sizes of the last run: valid points, voxels and kept voxels in total, and (nullable) per-frame offsets
 * [n_frames + 1] into the point / voxel / kept arrays. */
ot_status ot_rgbd_filter_sizes(const ot_rgbd_filter* filter, int64_t* points_host, int64_t* voxels_host,
                               int64_t* kept_host, int64_t* point_offsets_host, int64_t* voxel_offsets_host,
                               int64_t* kept_offsets_host);
/* Device arrays of the last run (valid until the next run / destroy; any out-pointer may be NULL): the kept
 * points xyz / rgb f64 [kept][3] and their index inside their frame's voxel cloud (int64, ascending per frame: the
 * indices remove_statistical_outlier returns), the voxel clouds xyz / rgb f64 [voxels][3] (per frame in key order,
 * as ot_voxel_down_sample) and every voxel's mean kNN distance f64 [voxels]. */
ot_status ot_rgbd_filter_outputs(const ot_rgbd_filter* filter, const double** kept_xyz, const double** kept_rgb,
                                 const int64_t** kept_index, const double** voxel_xyz, const double** voxel_rgb,
                                 const double** voxel_avg_dist);
/* Copy frame `frame`'s results (or every frame's, frame = -1) of the last run into caller device buffers, ordered on
 * `stream`; any pointer may be NULL.  Sizes: ot_rgbd_filter_sizes' offsets. */
ot_status ot_rgbd_filter_copy(const ot_rgbd_filter* filter, int32_t frame, double* kept_xyz, double* kept_rgb,
                              int64_t* kept_index, double* voxel_xyz, double* voxel_rgb, double* voxel_avg_dist,
                              void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Scalable TSDF volume — pipelines.integration.ScalableTSDFVolume (reconstruct_rgbd_filter.py:81-85)
 * ------------------------------------------------------------------------------------------------- */
typedef struct ot_tsdf ot_tsdf;

/* ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution=16,
 * depth_sampling_stride=4).  max_units is the INITIAL block-pool capacity in HBM (0 = default 32768 units): like
 * Open3D's volume the pool is unbounded -- a batch that needs more units grows the pool and the hash (records copied,
 * keys rehashed) and its dropped units are integrated again from the staged frames, bit-identical to a large pool;
 * only a failed device allocation is an error (OT_ERR_HIP, from the integrate / flush call whose batch needed it). */
ot_status ot_tsdf_create(double voxel_length, double sdf_trunc, int32_t color_type,
                         int32_t volume_unit_resolution, int32_t depth_sampling_stride, int64_t max_units,
                         ot_tsdf** out);
ot_status ot_tsdf_destroy(ot_tsdf* vol);
ot_status ot_tsdf_reset(ot_tsdf* vol);  /* ScalableTSDFVolume.reset() */
/* The same reset ordered on `stream` (no device-wide synchronisation): several volumes driven from several
 * host threads / streams do not stall each other.  Frames still queued for a batch are integrated first. */
ot_status ot_tsdf_reset_async(ot_tsdf* vol, void* stream);

/* volume.integrate(rgbd, intrinsic, extrinsic) — reconstruct_rgbd_filter.py:105.
 * depth: float32 [h][w] (already scaled/truncated); color: uint8 [h][w][3] (RGB8) or NULL (NoColor). */
ot_status ot_tsdf_integrate(ot_tsdf* vol, const float* depth, const uint8_t* color,
                            const ot_intrinsics* intrinsic, const double extrinsic[16], void* stream);

/* Fused RGBDImage.create_from_color_and_depth + integrate on raw uint16 depth (bit-identical to the
 * two-step path).  Frames are queued and integrated in batches (temporal blocking: each block is read
 * and written once per batch, voxels see frames in call order).  The queue is flushed by
 * ot_tsdf_flush, by any read of the volume and when it is full.  Input buffers must stay valid and
 * unmodified until the next flush returns (the Python facade keeps them alive). */
ot_status ot_tsdf_integrate_u16(ot_tsdf* vol, const uint16_t* depth, const uint8_t* color,
                                const ot_intrinsics* intrinsic, const double extrinsic[16],
                                double depth_scale, double depth_trunc, void* stream);
/* n frames of a scan already resident in device memory in one call: frame k's u16 depth at depth + k*W*H, its RGB8 at
 * color + 3*k*W*H (color may be NULL), its extrinsic at extrinsics + 16*k (host).  The same queueing, batching and
 * bits as n calls of ot_tsdf_integrate_u16, without n host round trips (the front of one object's latency); and when
 * the call leaves 64 frames or more queued (or the batch size, if smaller) their batch is started before it returns,
 * so a scan of 64..127 frames does not wait for the next reader under the default batch size of 128. */
ot_status ot_tsdf_integrate_u16_frames(ot_tsdf* vol, int32_t n, const uint16_t* depth, const uint8_t* color,
                                       const ot_intrinsics* in, const double* extrinsics, double depth_scale,
                                       double depth_trunc, void* stream);
ot_status ot_tsdf_flush(ot_tsdf* vol, void* stream);
/* Frames queued on the host for the next batch (their input buffers are still referenced; every frame queued before
 * them has been enqueued on its stream).  Host-only, no synchronisation. */
ot_status ot_tsdf_pending_frames(const ot_tsdf* vol, int32_t* n_host);
/* Batch size used by ot_tsdf_integrate_u16 (1 = integrate immediately).  Default and maximum 128 for a whole volume
 * whose batches run on the caller's stream; a sharded volume and the double-buffered, split and deferred front ends
 * batch by at most 64 whatever is set here.  A caller's frame must stay valid until its batch has run (the batch fills,
 * a flush or a reader): with the default that is up to 128 calls.  The first batch of more than 64 frames reallocates
 * the volume's staging to the batch size once (128 frames of 640 x 480: 315 MB, one stream synchronise). */
ot_status ot_tsdf_set_batch(ot_tsdf* vol, int32_t max_frames);
/* Double-buffered batch front end (spatial sharding of one object: reconstruct_rgbd_filter.py:88-109):
 * with mode 1 batch k+1's staging, touch and unit headers run on the caller's stream while batch k's integrate runs on
 * a second stream of the volume (two staging sets); readers (num_units, export, extraction, flush, reset) order the
 * caller's stream after the last integrate.  -1 (default): on for spatially sharded volumes (their split front end
 * stages only their units' tiles; measured faster at 2, 4 and 8 ranks), off otherwise; 0 off; 1 on.
 * Results are identical in every mode.  Fails with OT_ERR_INVALID_ARGUMENT while frames are queued (flush on their stream first).
 * A batch whose integrate is still deferred (sharded volumes from 4 ranks) need not be flushed first: the next batch
 * launches it before it restages anything. */
ot_status ot_tsdf_set_frontend_overlap(ot_tsdf* vol, int32_t mode);

/* Batch statistics since the last reset (measurement; not an Open3D API): integrate batches run, the units they touched
 * summed over batches, and how many of those were new in their batch (allocated by it: their state starts at zero and
 * is not read).  Frames still queued are not counted (flush first).  The bench's compulsory-bytes figure of the integrate kernel:
 * (2 x unit_batches - new_units) unit records + the staged pixels. */
ot_status ot_tsdf_batch_stats(ot_tsdf* vol, int64_t* batches, int64_t* unit_batches, int64_t* new_units);

/* Number of allocated volume units.  Queued frames are integrated first, on `stream`; synchronises `stream`. */
ot_status ot_tsdf_num_units(ot_tsdf* vol, int64_t* n_units_host, void* stream);
/* Cumulative voxel updates and volume-unit integrations since create/reset (flushes on `stream`, synchronises it). */
ot_status ot_tsdf_counters(ot_tsdf* vol, int64_t* voxel_updates_host, int64_t* unit_integrations_host,
                           void* stream);
/* Colour state precision: 64 (the default, as in the Python facade) keeps each voxel's running colour mean in float64
 * with exact IEEE division, as Open3D's TSDFVoxel::color_ (Eigen::Vector3d; reconstruct_rgbd_filter.py:81-85 ->
 * SURVEY A.3(iv)) -- bit-exact colours, 128-KiB unit records; 32 keeps float32 with one hardware reciprocal per update
 * (|rel| <= 1e-4, 80-KiB records, faster).  NoColor volumes keep no colour state whatever the setting (get reports
 * 32).  Call before the first integrate (the unit pool is reallocated when the record size changes). */
ot_status ot_tsdf_set_color_precision(ot_tsdf* vol, int32_t bits);
ot_status ot_tsdf_get_color_precision(const ot_tsdf* vol, int32_t* bits_host);

/* Kernel timing for roofline reporting: when enabled, HIP events bracket every launch of the dominant
 * integration kernel on the caller's stream; ot_tsdf_kernel_time returns the summed device time (ms) and the
 * number of timed launches since profiling was enabled (synchronises). */
ot_status ot_tsdf_set_profiling(ot_tsdf* vol, int32_t enable);
ot_status ot_tsdf_kernel_time(ot_tsdf* vol, double* total_ms_host, int64_t* launches_host);
/* The same for each batch's front end (frame staging + unit touch + unit headers): the work every rank of a
 * spatially sharded volume repeats for all pixels (bench.py's Amdahl bound of single-object sharding). */
ot_status ot_tsdf_frontend_time(ot_tsdf* vol, double* total_ms_host, int64_t* batches_host);

/* Dump every unit sorted by key (kx, ky, kz): keys int32 [U][3]; per unit 4096 voxels in Open3D
 * IndexOf order (x*256 + y*16 + z): tsdf f32, weight f32, color f32 [3] (0..255).  Any pointer may be
 * NULL.  Device pointers; every output holds `capacity` units. */
ot_status ot_tsdf_export_units(ot_tsdf* vol, int64_t capacity, int32_t* keys, float* tsdf, float* weight,
                               float* color, void* stream);
/* The colours as float64, [U][4096][3] in export_units' order: exact for a colour-precision-64 volume, the float32
 * state widened otherwise.  Both exports fail with OT_ERR_CAPACITY when the volume holds more than `capacity` units
 * (outputs sized from an older unit count).  A spatially sharded volume exports (and ot_tsdf_num_units counts) only
 * its own units, not the halo units ot_tsdf_import_border added. */
ot_status ot_tsdf_export_color64(ot_tsdf* vol, int64_t capacity, double* color, void* stream);

/* The inverse of ot_tsdf_export_units (same layouts): insert n units, overwriting any unit with the same key;
 * keys must be unique within one call.  color may be NULL (zeros).  Used to assemble a spatially sharded volume
 * on one GPU before extract_triangle_mesh.  Device pointers. */
ot_status ot_tsdf_import_units(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf, const float* weight,
                               const float* color, void* stream);
/* The same for a colour-precision-64 volume (float64 colours, export_color64's layout). */
ot_status ot_tsdf_import_units_color64(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf,
                                       const float* weight, const double* color, void* stream);

/* Spatial sharding of ONE object's volume over `world` GPUs (not an Open3D API): this volume
 * allocates and integrates only the units whose owner hash(key) mod world == rank.  Every rank integrates every
 * frame; each voxel still sees the frames in call order, so the union of the ranks' exported units is bit-identical
 * to one unsharded volume.  Call before the first integrate.  The hash is of the unit's ownership block (below). */
ot_status ot_tsdf_set_shard(ot_tsdf* vol, int32_t rank, int32_t world);
/* Ownership granularity of a sharded volume: blocks of 2^log2_units units per axis share one owner (the hash is taken
 * of the block key).  Set by ot_tsdf_set_shard to 2 (4^3 units) up to 4 ranks and 1 beyond; call after it, before the
 * first integrate. */
ot_status ot_tsdf_set_shard_block(ot_tsdf* vol, int32_t log2_units);
/* Sector ownership (round 6): the unit is owned by the azimuth sector (world equal sectors of the pseudo-angle; the true
 * 90 / 45 degree sectors at 4 / 8 ranks) of its centre around the scan centre (cx, cy) in metres -- for a ring scan the
 * look-at point, e.g. the ScanObject goal's x, y (otslam_interfaces/action/ScanObject.action) or the mean camera
 * position.  Each frame then sees a contiguous arc of a rank's units, so a sharded rank stages only the image tiles its
 * units project to (the split front end: tools/shard_sector_model.py).  Integer arithmetic on the unit
 * key only: results are exact for any centre.  Call instead of ot_tsdf_set_shard, before the first integrate. */
ot_status ot_tsdf_set_shard_sector(ot_tsdf* vol, int32_t rank, int32_t world, double cx, double cy);
/* Border-halo routing: per border row key int32 [n][3] (export_border's), the bitmask (bit r = rank r,
 * world <= 64) of the other ranks that own one of the unit's 7 -x/-y/-z neighbours -- the only ranks whose marching
 * cubes can read the row.  Device pointers; ordered on `stream`. */
ot_status ot_tsdf_border_destinations(const ot_tsdf* vol, int64_t n, const int32_t* keys, int64_t* dest_mask,
                                      void* stream);

/* Border halo of a spatially sharded volume (SURVEY §8(e) "all-gather of border faces"; not an Open3D API).
 * export_border: per OWN unit (sorted key order; halo units are not exported) its 721 low-face voxels (x == 0 ||
 * y == 0 || z == 0, increasing x*256 + y*16 + z): keys int32 [n][3], tsdf / weight f32 [n][721], colour
 * [n][721][3] in the volume's colour precision (f32, or f64 after ot_tsdf_set_color_precision(64); NULL to skip);
 * the row count to *n_exported_host (capacity: rows the buffers hold, ot_tsdf_num_units is enough).
 * import_border: rows of other shards; a row becomes a halo unit when its key is not owned by this shard and one of
 * its -x/-y/-z neighbours is (marching cubes of the own units reads exactly these voxels); other rows are skipped.
 * Marching cubes of a sharded volume then emits only the own units' cubes; ot_tsdf_fetch_mesh_keys gives the keys
 * that merge the shards' meshes into the unsharded mesh (distributed.extract_sharded_mesh). */
ot_status ot_tsdf_export_border(ot_tsdf* vol, int64_t capacity, int32_t* keys, float* tsdf, float* weight, void* color,
                                int64_t* n_exported_host, void* stream);
ot_status ot_tsdf_import_border(ot_tsdf* vol, int64_t n, const int32_t* keys, const float* tsdf, const float* weight,
                                const void* color, void* stream);

/* volume.extract_triangle_mesh() — reconstruct_rgbd_filter.py:112 (marching cubes, Appendix A.4).
 * Runs the extraction and stores the mesh inside the handle; returns its sizes.  Vertices are ordered by
 * (unit key, local voxel, edge) — a canonical order; Open3D's is hash order. */
ot_status ot_tsdf_extract_triangle_mesh(ot_tsdf* vol, int64_t* n_vertices_host, int64_t* n_triangles_host,
                                        void* stream);
/* Copy the extracted mesh out: vertices f64 [V][3], colors f64 [V][3] (0..1, NULL to skip),
 * triangles int32 [T][3].  Device pointers; ordered on `stream` (no synchronisation: the extraction and these copies
 * complete in stream order, before any later work on that stream). */
ot_status ot_tsdf_fetch_triangle_mesh(ot_tsdf* vol, double* vertices, double* vertex_colors,
                                      int32_t* triangles, void* stream);
/* The extraction in two phases, writing the mesh straight into the caller's arrays (no copy out of the volume's own
 * buffers): _count classifies, counts and returns the vertex / triangle totals (one read-back); _emit then writes
 * vertices [nv][3], vertex colours [nv][3] (may be NULL; zeros for NoColor) and triangles [nt][3] into device arrays
 * sized from those totals, in stream order.  _emit fails once the volume has changed since _count.  After a _count,
 * ot_tsdf_fetch_triangle_mesh emits again into its arguments (same bits) while the volume is unchanged;
 * ot_tsdf_fetch_mesh_keys needs one emission first. */
ot_status ot_tsdf_extract_triangle_mesh_count(ot_tsdf* vol, int64_t* n_vertices, int64_t* n_triangles, void* stream);
ot_status ot_tsdf_emit_triangle_mesh(ot_tsdf* vol, double* vertices, double* vertex_colors, int32_t* triangles,
                                     void* stream);
/* Count and emit in one call, for callers that can guess the size (e.g. the last extraction of this volume): the
 * emission into the given arrays (capacity_vertices / capacity_triangles rows) is queued before the totals are read
 * back, so the GPU does not wait for the host.  Returns OT_OK with the totals when they fit; otherwise
 * OT_ERR_CAPACITY with the totals set (rows past the capacities were not written): emit with
 * ot_tsdf_emit_triangle_mesh into arrays of that size. */
ot_status ot_tsdf_extract_triangle_mesh_into(ot_tsdf* vol, double* vertices, double* vertex_colors,
                                             int32_t* triangles, int64_t capacity_vertices, int64_t capacity_triangles,
                                             int64_t* n_vertices, int64_t* n_triangles, void* stream);
/* Serial of the last extraction (ot_tsdf_extract_triangle_mesh), or -1 once the volume has changed since (frames
 * integrated, reset, units imported). */
ot_status ot_tsdf_mesh_serial(const ot_tsdf* vol, int64_t* serial_host);
/* mesh.compute_vertex_normals() (reconstruct_rgbd_filter.py:113) of the mesh of extraction `serial`, whose
 * arrays (device pointers, unmodified) are passed: the same bits as ot_mesh_compute_vertex_normals, from the
 * marching-cubes structure kept with the volume (each vertex is a cut edge; its triangles are those of the <= 4 cubes
 * sharing it, walked in triangle order) instead of a sort of the 3T corners.  OT_ERR_INVALID_ARGUMENT when the volume
 * changed since that extraction or the sizes differ (take ot_mesh_compute_vertex_normals then).  Ordered on `stream`,
 * no synchronisation. */
ot_status ot_tsdf_mesh_vertex_normals(ot_tsdf* vol, int64_t serial, const double* vertices, int64_t n_vertices,
                                      const int32_t* triangles, int64_t n_triangles, double* out, void* stream);
/* Merge keys of the extracted mesh (device pointers, NULL to skip): per vertex int32 [V][4] = owner unit key
 * (x, y, z) and edge bit (local voxel x*256+y*16+z times 3 plus axis) -- the canonical vertex order; per triangle
 * int32 [T][3] = the unit key of its cube. */
ot_status ot_tsdf_fetch_mesh_keys(ot_tsdf* vol, int32_t* vertex_keys, int32_t* triangle_units, void* stream);

/* volume.extract_point_cloud() -- ScalableTSDFVolume::ExtractPointCloud: one point per grid edge
 * whose two usable voxels (weight != 0, tsdf in [-0.98, 0.98)) have tsdf of opposite sign, with the interpolated colour
 * and the normal of GetNormalAt (central differences of the trilinear tsdf).  Two phases like the mesh's: _count
 * integrates the queued frames, counts and returns the number of points (one read-back); _emit then writes points
 * f64 [n][3], normals f64 [n][3] and colours f64 [n][3] (0..1; NULL to skip; a NoColor volume has none and leaves the
 * array untouched) into device arrays of that size, in stream order.  Canonical order (Open3D's is hash order): unit
 * key, voxel x*256 + y*16 + z, axis.  _emit fails with OT_ERR_INVALID_ARGUMENT once the volume has changed since the
 * count.  The volume and its extracted mesh are left as they are.  A spatially sharded volume (ot_tsdf_set_shard,
 * ot_tsdf_set_shard_sector) is refused with OT_ERR_INVALID_ARGUMENT: the normals read units of other shards; extract
 * from the volume distributed.assemble_sharded_volume builds instead. */
ot_status ot_tsdf_extract_point_cloud_count(ot_tsdf* vol, int64_t* n_points_host, void* stream);
ot_status ot_tsdf_emit_point_cloud(ot_tsdf* vol, double* points, double* normals, double* colors, void* stream);
/* volume.extract_voxel_point_cloud() -- ScalableTSDFVolume::ExtractVoxelPointCloud: the centre
 * of every usable voxel, coloured (c, c, c) with c = (tsdf + 1) / 2; no normals.  The same two phases, order, refusal
 * of sharded volumes and validity as above (either count serves both emissions); points and colours f64 [n][3]. */
ot_status ot_tsdf_extract_voxel_point_cloud_count(ot_tsdf* vol, int64_t* n_points_host, void* stream);
ot_status ot_tsdf_emit_voxel_point_cloud(ot_tsdf* vol, double* points, double* colors, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Triangle meshes
 * ------------------------------------------------------------------------------------------------- */

/* mesh.compute_vertex_normals() — reconstruct_rgbd_filter.py:113 (Appendix A.5). */
ot_status ot_mesh_compute_vertex_normals(const double* vertices, int64_t n_vertices,
                                         const int32_t* triangles, int64_t n_triangles, double* out_normals,
                                         void* stream);

/* mesh.sample_points_uniformly(number_of_points) — reconstruct_rgbd_filter.py:123 (Appendix A.8), with a
 * seeded counter-based RNG (Open3D's is unseeded).  normals / colors may be NULL. */
ot_status ot_mesh_sample_points_uniformly(const double* vertices, const double* vertex_normals,
                                          const double* vertex_colors, int64_t n_vertices,
                                          const int32_t* triangles, int64_t n_triangles, int64_t n_points,
                                          uint64_t seed, double* out_xyz, double* out_normals,
                                          double* out_colors, void* stream);

/* mesh.get_surface_area() — Open3D TriangleMesh::GetSurfaceArea, the first of SamplePointsUniformly's two serial
 * float64 chains (reconstruct_rgbd_filter.py:123): ((0 + a_0) + a_1) + ... over the triangle areas in index order,
 * bit-exact.  area_host: host double. */
ot_status ot_mesh_get_surface_area(const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                   int64_t n_triangles, double* area_host, void* stream);

/* The same sampling for several meshes in one call (e.g. the objects of a multi-object run on one GPU): results
 * are identical to one ot_mesh_sample_points_uniformly call per mesh; the meshes' area sums and CDFs are computed
 * side by side.  jobs_host: host array; every pointer inside is a device pointer. */
typedef struct ot_mesh_sample_job {
    const double* vertices;
    const double* vertex_normals;  /* may be NULL */
    const double* vertex_colors;   /* may be NULL */
    int64_t n_vertices;
    const int32_t* triangles;
    int64_t n_triangles;
    double* out_xyz;               /* [n_points][3] */
    double* out_normals;           /* may be NULL */
    double* out_colors;            /* may be NULL */
} ot_mesh_sample_job;
ot_status ot_mesh_sample_points_uniformly_batch(const ot_mesh_sample_job* jobs_host, int32_t n_jobs,
                                                int64_t n_points, uint64_t seed, void* stream);
/* The same, with a hipEvent_t (nullable) that the point emission waits for: the area sums and CDFs read only the
 * vertices and triangles and start at once, while the vertex normals (or colours) the emission interpolates may
 * still be computed on another stream (the facade's compute_vertex_normals of a fresh mesh,
 * reconstruct_rgbd_filter.py:113 -> :123). */
ot_status ot_mesh_sample_points_uniformly_after(const ot_mesh_sample_job* jobs_host, int32_t n_jobs,
                                                int64_t n_points, uint64_t seed, void* inputs_ready_event,
                                                void* stream);
/* reconstruct_rgbd_filter.py:123-132 in one pass per mesh: sample_points_uniformly(n_points) (the same points as
 * ot_mesh_sample_points_uniformly with this seed), then the Z mask points[:, 2] >= z_min (NaN fails) applied in
 * the sampling order.  The reference rebuilds its cloud from the points and colours alone, so the kept rows are written
 * to out_xyz / out_colors (each with room for n_points rows; out_colors may be NULL) and normals are not interpolated
 * (out_normals and vertex_normals are ignored: the vertex normals need not be ready).  n_kept_host: host int64_t
 * [n_jobs], the kept row count of each job.  Synchronises the stream. */
ot_status ot_mesh_sample_points_min_z(const ot_mesh_sample_job* jobs_host, int32_t n_jobs, int64_t n_points,
                                      uint64_t seed, double z_min, int64_t* n_kept_host, void* stream);
/* reconstruct_rgbd_filter.py:112-132 of one volume in ONE host call (replaces the facade's extract_triangle_mesh ->
 * compute_vertex_normals -> sample_points_uniformly + Z-mask sequence at :112-132; no host work between the
 * marching-cubes totals and the sampler's first launch): the mesh into vertices / vertex_colors / triangles with the
 * given capacities exactly as ot_tsdf_extract_triangle_mesh_into, then ot_mesh_sample_points_min_z of it (n_points,
 * seed, z_min; kept rows into out_xyz / out_rgb, each with room for n_points rows; out_rgb may be NULL), and its vertex
 * normals (ot_tsdf_mesh_vertex_normals, bit-identical to ot_mesh_compute_vertex_normals) into vertex_normals (NULL:
 * none) on normals_stream beside the sampling -- a reader of the normals orders itself after normals_stream.
 * OT_ERR_CAPACITY: the mesh did not fit; *n_vertices / *n_triangles are its size, nothing was sampled (emit it with
 * ot_tsdf_emit_triangle_mesh and sample it separately).  An empty mesh samples nothing (*n_kept_host = 0).
 * Synchronises `stream`. */
ot_status ot_tsdf_extract_sample_min_z(ot_tsdf* vol, double* vertices, double* vertex_colors, int32_t* triangles,
                                       int64_t capacity_vertices, int64_t capacity_triangles, double* vertex_normals,
                                       void* normals_stream, int64_t n_points, uint64_t seed, double z_min,
                                       double* out_xyz, double* out_rgb, int64_t* n_vertices_host,
                                       int64_t* n_triangles_host, int64_t* n_kept_host, void* stream);
/* The same in two calls: _async queues the sampling and returns without synchronising (the output arrays must stay
 * allocated), _wait synchronises it and fills n_kept_host.  Between them the calling thread may queue other work (the
 * facade queues a fresh mesh's deferred vertex normals there, beside the sampling's walks) but no other sampling. */
ot_status ot_mesh_sample_points_min_z_async(const ot_mesh_sample_job* jobs_host, int32_t n_jobs, int64_t n_points,
                                            uint64_t seed, double z_min, void* stream);
ot_status ot_mesh_sample_points_min_z_wait(int32_t n_jobs, int64_t* n_kept_host);

/* Connected components and triangle clean-up ("mesh components").  Every pointer is a device pointer
 * unless its name ends in _host.  Every entry checks its arguments before any device work (NULL buffers, negative
 * sizes, 3 n_triangles or n_vertices beyond 31 bits: OT_ERR_INVALID_ARGUMENT), and every entry that takes n_vertices
 * first checks the triangle array alone: an index outside [0, n_vertices) gives OT_ERR_INVALID_ARGUMENT ("triangle
 * index out of range") before that index addresses anything.  All synchronise `stream`.
 *
 * mesh.cluster_connected_triangles() — TriangleMesh::ClusterConnectedTriangles.  Triangle (a, b, c) has the edge keys
 * (min, max) of (a, b), (b, c), (c, a), (a, a) of a degenerate triangle included; two triangles are adjacent when they
 * share an edge key (sharing one vertex only is not adjacency); the clusters are the connected components of that
 * adjacency, numbered 0 .. C-1 by ascending smallest triangle index (the labels of Open3D's index-order fill).
 * out_triangle_clusters [T]; out_cluster_n_triangles [capacity T], the first C written; out_cluster_area [capacity T]
 * (NULL exactly when vertices is NULL: no areas), the first C written: the float64 sum of the cluster's triangle areas
 * (TriangleMesh::GetTriangleArea) in an association fixed by the cluster's size, over its triangles in ascending
 * index order -- the same bits from call to call; a cluster of one triangle gets that triangle's area unchanged. */
ot_status ot_mesh_cluster_connected_triangles(const int32_t* triangles, int64_t n_triangles,
                                              const double* vertices /* nullable */, int64_t n_vertices,
                                              int32_t* out_triangle_clusters, int32_t* out_cluster_n_triangles,
                                              double* out_cluster_area /* nullable */, int64_t* n_clusters_host,
                                              void* stream);
/* mesh.remove_degenerate_triangles(): out_remove_mask[t] = 1 when two of the triangle's three indices are equal,
 * else 0. */
ot_status ot_mesh_flag_degenerate_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                            uint8_t* out_remove_mask /* [T] */, void* stream);
/* mesh.remove_duplicated_triangles(): the canonical key of (t0, t1, t2) is, if t0 <= t1, (t0, t1, t2) when t0 <= t2
 * else (t2, t0, t1); otherwise (t1, t2, t0) when t1 <= t2 else (t2, t0, t1).  out_remove_mask[t] = 1 when an earlier
 * triangle has the same key, else 0 (rotations are duplicates, flips are not). */
ot_status ot_mesh_flag_duplicated_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                            uint8_t* out_remove_mask /* [T] */, void* stream);
/* mesh.remove_triangles_by_mask(mask): the triangles whose mask byte is 0, in order, into out_triangles (room for T
 * rows, must not alias triangles); *n_kept_host their number. */
ot_status ot_mesh_remove_triangles_by_mask(const int32_t* triangles, int64_t n_triangles, const uint8_t* remove_mask,
                                           int32_t* out_triangles, int64_t* n_kept_host, void* stream);
/* mesh.remove_unreferenced_vertices(): out_kept_old_index [capacity V] receives, ascending, the vertices that occur in
 * some triangle (*n_kept_host of them); the triangle indices are rewritten IN PLACE to the new numbering.  The caller
 * gathers vertices, colours and normals by that index (ot_gather_rows3). */
ot_status ot_mesh_remove_unreferenced_vertices(int64_t n_vertices, int32_t* triangles_inout, int64_t n_triangles,
                                               int32_t* out_kept_old_index, int64_t* n_kept_host, void* stream);

/* Adjacency, smoothing / sharpening filters and vertex clustering ("mesh filters").  Device pointers
 * unless the name ends in _host; arguments are checked before any device work, and an entry that takes triangles
 * refuses an index outside [0, n_vertices) before anything else runs ("[<Call>] triangle index out of range
 * [0, n_vertices)").
 *
 * mesh.compute_adjacency_list() as a CSR: for every triangle (a, b, c), b and c are neighbours of a, a and c of b, a
 * and b of c; repeats collapse, and (a, a, b) makes a its own neighbour.  out_offsets int32 [n_vertices + 1];
 * out_neighbours int32 [capacity 6 n_triangles], row v = [offsets[v], offsets[v + 1]) in ascending neighbour index;
 * *n_entries_host = offsets[n_vertices].  6 n_triangles must fit 31 bits.  Synchronises. */
ot_status ot_mesh_compute_adjacency(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                    int32_t* out_offsets, int32_t* out_neighbours, int64_t* n_entries_host,
                                    void* stream);
/* mesh.filter_smooth_simple / _laplacian / _taubin / filter_sharpen over that CSR (n_entries = offsets[n_vertices]; a
 * CSR that does not fit n_vertices is refused).  kind: 0 simple, 1 Laplacian (p0 = lambda), 2 Taubin (p0 = lambda,
 * p1 = mu: each iteration a Laplacian step with lambda, then one with mu), 3 sharpen (p0 = strength).  scope: bit 0
 * vertices, bit 1 normals, bit 2 colours.  An attribute is filtered when its scope bit is set and its input is not
 * NULL, and copied to its output otherwise; iterations <= 0 copies everything.  N(v) in ascending index, n = |N(v)|,
 * every sum one left-to-right float64 chain, every step reading the previous step's values only:
 *   simple     s = x[v]; s += x[w]...; x'[v] = s / (1 + n)
 *   Laplacian  wt = 1 / (|p[v] - p[w]| + 1e-12) from the previous positions; W += wt, S += wt x[w] from 0;
 *              x'[v] = x[v] + lambda (S / W - x[v])
 *   sharpen    s += x[w] from 0; x'[v] = x[v] (1 + strength n) - strength s
 * A vertex without neighbours keeps its attributes.  Outputs must not alias inputs; an output is required for every
 * input given.  Ordered on `stream`. */
ot_status ot_mesh_filter(int32_t kind, const double* vertices, const double* normals /* nullable */,
                         const double* colors /* nullable */, int64_t n_vertices, const int32_t* offsets,
                         const int32_t* neighbours, int64_t n_entries, int32_t iterations, double p0, double p1,
                         int32_t scope, double* out_vertices, double* out_normals, double* out_colors, void* stream);
/* mesh.simplify_vertex_clustering(voxel_size, contraction): contraction 0 = Average (1 = Quadric is refused).  Voxel
 * key floor((p - (min_bound - voxel_size / 2)) / voxel_size) per axis in float64, with ot_voxel_down_sample's
 * refusals ("voxel_size <= 0.", "voxel_size is too small.").  New vertex k is the k-th voxel by first appearance in
 * ascending old vertex index; its position, normal and colour are the sums over its old vertices in ascending index,
 * from 0, divided by their number (normals not normalised).  A triangle whose mapped corners are not all different is
 * dropped; the others are rotated to start at their smallest index, and one per distinct triple is kept (a flip is
 * another triple), in ascending index of the first source triangle.  out_vertices / out_normals / out_colors have room
 * for n_vertices rows, out_triangles for n_triangles.  Synchronises. */
ot_status ot_mesh_simplify_vertex_clustering(const double* vertices, const double* normals /* nullable */,
                                             const double* colors /* nullable */, int64_t n_vertices,
                                             const int32_t* triangles, int64_t n_triangles, double voxel_size,
                                             int32_t contraction, double* out_vertices, double* out_normals,
                                             double* out_colors, int64_t* n_out_vertices_host, int32_t* out_triangles,
                                             int64_t* n_out_triangles_host, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Hybrid map — fusion/hybrid_map.py
 * ------------------------------------------------------------------------------------------------- */

/* create_map_cloud (hybrid_map.py:25-60): occupied pixels (img < threshold) in row-major order →
 * (ox + c*res, oy + (h-1-r)*res, 0).  img: uint8 [h][w].  out_xyz holds h*w rows. */
ot_status ot_occupancy_to_points(const uint8_t* img, int32_t height, int32_t width, int32_t threshold,
                                 double resolution, double origin_x, double origin_y, double* out_xyz,
                                 int64_t* n_out_host, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Change detection against a saved map (BASELINE configs[4])
 * ------------------------------------------------------------------------------------------------- */

/* 2d_selective_merge.py:58-69 smart_paste(base_img, overlay_img, x, y, w, h), in place on device uint8
 * [height][width] grids: inside the rectangle, cells of `overlay` outside [unknown - threshold,
 * unknown + threshold] (205 ± 5 in the reference) overwrite `base`.  A rectangle reaching outside the image
 * leaves `base` unchanged (:59-60).  n_changed_host (optional) = cells whose value changed. */
ot_status ot_grid_smart_paste(uint8_t* base, const uint8_t* overlay, int32_t height, int32_t width, int32_t x,
                              int32_t y, int32_t w, int32_t h, int32_t unknown, int32_t threshold,
                              int64_t* n_changed_host, void* stream);

/* Voxel-key set difference of a new cloud against a saved cloud on the lattice floor((p - origin) / voxel_size)
 * (origin: host double[3]).  out_added = keys of `new` absent from `old`, out_removed = keys of `old` absent
 * from `new`, each int32 [k][3] sorted lexicographically (capacity: the cloud's point count). */
ot_status ot_voxel_key_diff(const double* new_xyz, int64_t n, const double* old_xyz, int64_t m, double voxel_size,
                            const double origin[3], int32_t* out_added, int64_t* n_added_host,
                            int32_t* out_removed, int64_t* n_removed_host, void* stream);

/* The same for n_objects objects at once (a hybrid map's object clouds vs their saved versions): clouds are
 * concatenated, object j = rows [offsets[j], offsets[j+1]) (host offsets, n_objects + 1 each); outputs are
 * int32 [k][4] = (object, x, y, z), sorted by object then key.  Lattice coordinates must lie in (-2^30, 2^30)
 * and the joint extent plus the object id must pack into 64 bits; at most 2048 objects.  Equals n_objects calls
 * of ot_voxel_key_diff. */
ot_status ot_voxel_key_diff_multi(const double* new_xyz, const int64_t* new_offsets, const double* old_xyz,
                                  const int64_t* old_offsets, int32_t n_objects, double voxel_size,
                                  const double origin[3], int32_t* out_added, int64_t* n_added_host,
                                  int32_t* out_removed, int64_t* n_removed_host, void* stream);

/* diff_node.cpp:103-160 ChangeDetectorNode::scanCallback, batched: n_scans pairs of float ranges
 * [n_scans][n_beams] (real scan, virtual scan of the saved map).  Per beam: new_flags = a real return with no
 * virtual return within +-search_window beams closer than distance_threshold; gone_flags = the converse.
 * Flagged beams are moved to the map frame with poses_host[n_scans][7] = (tx, ty, tz, qx, qy, qz, qw) and
 * binned to (int)(p / grid_resolution) cells (int32 [n_scans][n_beams][2]; 0 where not flagged). */
ot_status ot_scan_diff(const float* real_ranges, const float* virtual_ranges, int32_t n_scans, int32_t n_beams,
                       float real_angle_min, float real_angle_increment, float real_range_max,
                       float virtual_angle_min, float virtual_angle_increment, double distance_threshold,
                       int32_t search_window, const double* poses_host, double grid_resolution, uint8_t* new_flags,
                       uint8_t* gone_flags, int32_t* new_keys, int32_t* gone_keys, void* stream);

/* virtual_scan_node.cpp:245-292 publish_virtual_scan, batched: the saved map (OccupancyGrid int8 [height][width],
 * 100 = occupied; resolution / origin as the message's float fields) ray-marched per beam in steps of one
 * resolution from each robot pose (poses_host [n_scans][3] = x, y, yaw — yaw as tf2::getYaw); out_ranges float32
 * [n_scans][n_beams], +inf where no occupied cell is met before range_max or the map edge. */
ot_status ot_virtual_scan(const int8_t* grid, int32_t height, int32_t width, float resolution, float origin_x,
                          float origin_y, int32_t n_scans, int32_t n_beams, float angle_min, float angle_increment,
                          float range_max, const double* poses_host, float* out_ranges, void* stream);

/* diff_node.cpp:163-185 updateGrid / :188-222 publishCloud: time-decayed evidence grid (host state). */
typedef struct ot_change_grid ot_change_grid;
ot_status ot_change_grid_create(double time_threshold, double decay_rate, double grid_resolution,
                                ot_change_grid** out);
ot_status ot_change_grid_destroy(ot_change_grid* grid);
/* one scan: cells of the flagged beams (host keys [n][2], flags [n]) += dt (capped at 1.5 time_threshold);
 * all other cells -= decay_rate * dt; cells at <= 0 are erased. */
ot_status ot_change_grid_update(ot_change_grid* grid, const int32_t* keys_host, const uint8_t* flags_host,
                                int64_t n, double dt);
/* cells above time_threshold as float32 (x*res + res/2, y*res + res/2, 0), sorted by (x, y); out may be NULL
 * to query the count. */
ot_status ot_change_grid_publish(const ot_change_grid* grid, float* out_xyz_host, int64_t capacity,
                                 int64_t* n_host);

/* ---------------------------------------------------------------------------------------------------
 * Object trigger: scan clustering, object map filter, goal observations (DESIGN.md §4 "scan clustering")
 * ------------------------------------------------------------------------------------------------- */

/* The parameters of LidarClusterPublisher (lidar_cluster_publisher.cpp:73-102) with the node's defaults
 * 0.2, 1, 1.0, 1.0, 2.0, 0.001, 1, 20; held as float / int as the node's members are. */
typedef struct ot_scan_cluster_params {
    float gap_threshold;
    int32_t min_cluster_points;
    float max_range_ratio;
    float obj_len_max;
    float wal_len_min;
    float wal_lin_max;
    int32_t obj_nmp_min;
    int32_t wal_nmp_min;
} ot_scan_cluster_params;

#define OT_SCAN_CLASS_NONE 0
#define OT_SCAN_CLASS_WALL 1
#define OT_SCAN_CLASS_OBJECT 2
#define OT_SCAN_CLASS_UNKNOWN 3
#define OT_SCAN_CLUSTER_MAX_BEAMS 4096

/* one row of the cluster table (24 bytes) */
typedef struct ot_scan_cluster_row {
    int32_t first_beam; /* beam of the cluster's first stored point (seam-merged: the last cluster's first) */
    int32_t n_points;
    float length;  /* bounding-box diagonal, float as the node */
    int32_t cls;   /* OT_SCAN_CLASS_* */
    double linearity; /* float64 definition of DESIGN.md §4 */
} ot_scan_cluster_row;

/* lidar_cluster_publisher.cpp:151-291 LidarClusterPublisher::scanCallback, batched over n_scans scans of device
 * float ranges [n_scans][n_beams], 0 < n_beams <= OT_SCAN_CLUSTER_MAX_BEAMS (one workgroup stages a scan in LDS;
 * more beams -> OT_ERR_INVALID_ARGUMENT).  A beam is valid when finite and <= range_max * max_range_ratio
 * (:162-163); consecutive valid beams further apart than gap_threshold (hypotf, :172-173) start a new cluster;
 * clusters below min_cluster_points are dropped (:175, :182); the last and first kept clusters merge across the
 * seam when their end points are closer than gap_threshold (:186-199; a single kept cluster is kept once — the
 * node's self-insert is undefined); each cluster is WALL / OBJECT / UNKNOWN by :245-256 from its float length,
 * its linearity (float64 definition) and its point count.  min_cluster_points < 1 is refused (with 0
 * the node pushes an empty cluster for a scan without valid beams).  poses_host [n_scans][7] = (tx, ty, tz,
 * qx, qy, qz, qw) map <- base_link, NULL = identity.  Device outputs: beam_cluster int32 [n_scans][n_beams]
 * (index in the node's final cluster list, -1 = none), beam_class uint8 (OT_SCAN_CLASS_*), beam_xy float32
 * [n_scans][n_beams][2] (map frame, :265-274: the double transform cast to float; NaN for invalid beams),
 * n_clusters int32 [n_scans], clusters [n_scans][n_beams] rows (the first n_clusters of a scan are written).
 * The three published clouds (:287-290), float32 xyz with z = 0, are written concatenated over scans in the
 * node's order (cluster-list order, stored order inside a cluster) into wall_xyz / object_xyz / unknown_xyz
 * (capacity n_scans * n_beams rows each); cloud_offsets_host int64 [3][n_scans + 1] (wall, object, unknown)
 * receives their per-scan row offsets. */
ot_status ot_scan_cluster(const float* ranges, int32_t n_scans, int32_t n_beams, float angle_min,
                          float angle_increment, float range_max, const double* poses_host,
                          const ot_scan_cluster_params* params, int32_t* beam_cluster, uint8_t* beam_class,
                          float* beam_xy, int32_t* n_clusters, ot_scan_cluster_row* clusters, float* wall_xyz,
                          float* object_xyz, float* unknown_xyz, int64_t* cloud_offsets_host, void* stream);

/* object_filter.cpp:51-155 ObjectMapFilter, batched: object points float32 xyz, concatenated, scan s = rows
 * [offsets_host[s], offsets_host[s+1]).  The wall points of scan s come from virtual_ranges[s] (device float
 * [n_scans][n_beams]; NaN, inf and r > range_max skipped, :66), moved to the map frame by the yaw of
 * poses_host[s] (:157-172; NULL = identity).  A point is kept when no wall point lies closer than
 * proximity_threshold (:120-127: float differences and squares, compared in double); a scan without wall
 * points keeps nothing (:93).  keep_mask uint8 [n_points]; out_xyz the kept points in input order (capacity
 * n_points rows); out_offsets_host int64 [n_scans + 1] their per-scan offsets. */
ot_status ot_object_map_filter(const float* object_xyz, const int64_t* offsets_host, int32_t n_scans,
                               const float* virtual_ranges, int32_t n_beams, float angle_min, float angle_increment,
                               float range_max, const double* poses_host, double proximity_threshold,
                               uint8_t* keep_mask, float* out_xyz, int64_t* out_offsets_host, void* stream);

/* The parameters of the goal selector's clustering (3_multi_object_goal_selector.cpp:41-45), defaults 0.4, 10,
 * 0.2, 0.5. */
typedef struct ot_observation_params {
    double cluster_distance_threshold;
    double wall_thickness_threshold;
    double lock_margin;
    int32_t min_cluster_points;
} ot_observation_params;

/* 3_multi_object_goal_selector.cpp:172-215 cloudCallback's front half, batched over n_clouds clouds: points are
 * device float32 rows of point_stride floats (x, y first; 2 or 3), cloud j = rows [offsets_host[j],
 * offsets_host[j+1]) in message order, at most OT_SCAN_CLUSTER_MAX_BEAMS rows each.  Consecutive points further
 * apart than cluster_distance_threshold split clusters (:181-189, no seam merge); clusters below
 * min_cluster_points are dropped; clusters whose bounding box is thinner than wall_thickness_threshold are
 * skipped (:200).  Each remaining cluster gives one row (cx, cy, width, height, lock_radius) as float: the box
 * midpoint through poses_host[j] (global <- cloud frame, NULL = identity), lock_radius = diagonal / 2 +
 * lock_margin (:134-137).  Rows of cloud j start at out_rows + 5 * offsets_host[j] (capacity: 5 floats per input
 * point); n_obs_host int32 [n_clouds] receives their counts. */
ot_status ot_cluster_observations(const float* points, int32_t point_stride, const int64_t* offsets_host,
                                  int32_t n_clouds, const double* poses_host, const ot_observation_params* params,
                                  float* out_rows, int32_t* n_obs_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OTSLAM_H */
