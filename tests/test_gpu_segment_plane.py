"""GPU parity of PointCloud.segment_plane (csrc/segment_plane.hip) against the numpy restatement in
tests/segment_plane_ref.py: the plane bit for bit, the inlier indices, and the iterations the loop counted.  Every
cloud has at most 5 000 points; the designed clouds are those of tests/segment_plane_clouds.py, whose properties
test_segment_plane_api.py asserts on the CPU."""
import numpy as np
import pytest

import dbscan_ref as DB
import segment_plane_clouds as SC
import segment_plane_ref as SP
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu


def _pcd(pkg, pts):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.ascontiguousarray(pts, np.float64))
    return p


def _gpu(pkg, pts, thr, rn=3, iters=100, prob=0.99999999, seed=0):
    cloud = _pcd(pkg, pts)
    plane, inl = cloud.segment_plane(thr, rn, iters, prob, seed)
    assert isinstance(plane, np.ndarray) and plane.dtype == np.float64 and plane.shape == (4,)
    assert isinstance(inl, pkg.utility.IntVector) and all(type(v) is int for v in inl[:16])
    return plane, np.asarray(inl, np.int64).reshape(-1), cloud._segment_plane_evaluated


def _check(pkg, pts, thr, rn=3, iters=100, prob=0.99999999, seed=0, what=""):
    assert len(pts) <= 5000
    ref = SP.segment_plane(pts, thr, rn, iters, prob, seed)
    plane, inl, evaluated = _gpu(pkg, pts, thr, rn, iters, prob, seed)
    assert_bitwise(inl, ref.inliers, f"{what}: inliers")
    assert_bitwise(plane, ref.plane, f"{what}: plane")
    assert evaluated == ref.evaluated, f"{what}: {evaluated} iterations counted, reference {ref.evaluated}"
    return ref


def test_segment_plane_random_clouds(pkg, gpu):
    broke = 0
    for name, pts, thr, rn, iters, prob, seed in SC.random_cases():
        ref = _check(pkg, pts, thr, rn, iters, prob, seed, name)
        broke += ref.broke
    assert 0 < broke < len(SC.RANDOM_PARAMS)


def test_segment_plane_runs_through_several_chunks(pkg, gpu):
    for name, pts, thr, rn, iters, prob, seed in SC.long_run_cases():
        ref = _check(pkg, pts, thr, rn, iters, prob, seed, name)
        assert ref.evaluated > 256


def test_segment_plane_point_counts(pkg, gpu):
    for name, pts, thr, rn in SC.size_cases():
        ref = _check(pkg, pts, thr, rn, what=name)
        assert len(ref.inliers) >= 3


def test_segment_plane_equal_count_slabs(pkg, gpu):
    decided = 0
    for seed in range(4):
        ref = _check(pkg, SC.slabs_exact_and_jittered(), SC.SLAB_THRESHOLD, seed=seed,
                     what=f"exact and jittered slab, seed {seed}")
        decided += ref.rmse_decided
        ref = _check(pkg, SC.slabs_both_exact(), SC.SLAB_THRESHOLD, seed=seed, what=f"two exact slabs, seed {seed}")
        assert ref.ties >= 1 and ref.rmse_decided == 0
    assert decided >= 1


def test_segment_plane_points_at_exactly_the_threshold(pkg, gpu):
    pts, raised = SC.at_threshold()
    lo = _check(pkg, pts, 0.25, what="threshold 0.25")
    hi = _check(pkg, pts, np.nextafter(0.25, 1.0), what="threshold nextafter(0.25, 1)")
    assert not set(raised) & set(lo.inliers.tolist()) and set(raised) <= set(hi.inliers.tolist())


def test_segment_plane_degenerate_cloud(pkg, gpu):
    ref = _check(pkg, SC.degenerate(), 0.01, iters=200, what="degenerate cloud")
    assert ref.skipped >= 20


def test_segment_plane_all_points_on_one_plane(pkg, gpu):
    ref = _check(pkg, SC.one_plane(), 0.01, what="one exact plane")
    assert ref.evaluated == 1 and len(ref.inliers) == 500


def test_segment_plane_offset_cloud(pkg, gpu):
    _check(pkg, SC.offset_cloud(), SC.THRESHOLD, what="cloud shifted by (1000, -2000, 500) m")


def test_segment_plane_edge_values(pkg, gpu):
    """No inliers (distance_threshold = 0, num_iterations = 0): an empty list, and the model GetPlaneFromPoints gives
    for no points.  The definition's formulas give the zero plane there, not NaNs: the centroid is 0 / 0, but every
    moment sum is empty, so abc = 0, and the `norm == 0` branch returns (0, 0, 0, 0) before the centroid is used.
    The reference states the formulas literally and the GPU result must match it bit for bit."""
    pts = SC.plane_and_noise(77, 500, 0.6)
    for thr, iters in ((0.0, 100), (SC.THRESHOLD, 0), (SC.THRESHOLD, -5)):
        ref = _check(pkg, pts, thr, iters=iters, what=f"threshold {thr}, {iters} iterations")
        assert len(ref.inliers) == 0
    ref = _check(pkg, pts, SC.THRESHOLD, prob=1.0, what="probability 1")
    assert ref.evaluated + ref.skipped == 100 and not ref.broke


def test_segment_plane_is_deterministic(pkg, gpu):
    pts = SC.plane_and_noise(91, 5000, 0.5)
    a = _gpu(pkg, pts, SC.THRESHOLD, seed=1)
    b = _gpu(pkg, pts, SC.THRESHOLD, seed=1)
    assert_bitwise(a[0], b[0], "the same call twice: plane")
    assert_bitwise(a[1], b[1], "the same call twice: inliers")
    assert a[2] == b[2]
    planes = [_check(pkg, pts, SC.THRESHOLD, seed=s, what=f"seed {s}").plane for s in (1, 2)]
    assert (planes[0] != planes[1]).any()


def test_segment_plane_then_dbscan_on_a_surface_cloud(pkg, synth, seq16, gpu):
    """one frame of the package's own pipeline: unproject, voxel_down_sample, take the floor out, cluster the rest"""
    depth, color, ext = seq16
    intr = pkg.camera.PinholeCameraIntrinsic(*ref_intr(synth))
    rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(color[0]), pkg.geometry.Image(depth[0]), depth_scale=1000.0, depth_trunc=5.0,
        convert_rgb_to_intensity=False)
    ds = pkg.geometry.PointCloud.create_from_rgbd_image(rgbd, intr, ext[0]).voxel_down_sample(0.05)
    pts = np.asarray(ds.points).reshape(-1, 3)
    assert 500 < len(pts) <= 5000
    plane, inliers = ds.segment_plane(0.02, ransac_n=3, num_iterations=100, seed=5)
    ref = SP.segment_plane(pts, 0.02, 3, 100, seed=5)
    assert_bitwise(plane, ref.plane, "surface cloud: plane")
    assert_bitwise(np.asarray(inliers, np.int64).reshape(-1), ref.inliers, "surface cloud: inliers")
    assert ds._segment_plane_evaluated == ref.evaluated
    print(f"surface cloud: {len(pts)} points, plane {plane}, {len(inliers)} floor points, "
          f"{ref.evaluated} iterations counted")
    assert abs(plane[2]) > 0.99 and len(inliers) > 100
    rest = ds.select_by_index(inliers, invert=True)
    keep = np.ones(len(pts), bool)
    keep[ref.inliers] = False
    assert_bitwise(np.asarray(rest.points).reshape(-1, 3), pts[keep], "surface cloud: the remainder")
    labels = np.asarray(rest.cluster_dbscan(0.07, 6), np.int32)
    assert_bitwise(labels, DB.cluster_dbscan(pts[keep], 0.07, 6), "surface cloud: DBSCAN(0.07, 6) on the remainder")
