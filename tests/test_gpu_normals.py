"""GPU parity of PointCloud.estimate_covariances / estimate_normals / the orientation calls (csrc/normals.hip over the
grid of csrc/grid.h) against the exhaustive float64 reference of tests/normals_ref.py on the designed clouds of
tests/normals_clouds.py (at most 5 000 points each; test_normals_api.py asserts their properties on the CPU).

Bit for bit: every covariance; the normals of every point whose reference path is 0, 1 or 2 (no library call on those
paths); the orientation calls and normalize_normals on identical inputs.  Trigonometric-path normals (acos and cos
come from the device library) are compared up to sign by angle where the reference gap is >= 1e-3, within 16 x the
reference's own float64-vs-long-double angle over those points, at least 64 * 2^-53 (normals_clouds.tolerance)."""
import numpy as np
import pytest

import normals_clouds as NC
import normals_ref as NR
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu


def _pcd(pkg, pts, normals=None):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.ascontiguousarray(pts, np.float64))
    if normals is not None:
        p.normals = pkg.utility.Vector3dVector(np.ascontiguousarray(normals, np.float64))
    return p


def _param(pkg, k, radius):
    g = pkg.geometry
    return g.KDTreeSearchParamKNN(k) if radius is None else g.KDTreeSearchParamHybrid(radius, k)


def _estimate(pkg, name):
    pts, k, radius, prior = NC.cases()[name]
    p = _pcd(pkg, pts, prior)
    assert p.estimate_normals(_param(pkg, k, radius)) is None
    assert p.has_normals() and p.has_covariances()
    return p, np.array(p.normals), np.array(p.covariances)


def _compare_normals(got, ref, what, exempt=False):
    det = ref["path"] != NR.PATH_TRIG
    assert_bitwise(got[det], ref["normals"][det], f"{what}: normals of the paths without a library call")
    mask, limit, worst = NC.tolerance(ref)
    left_out = int(((~det) & ~mask).sum())
    ang = NR.angle(got[mask], ref["normals"][mask]) if mask.any() else np.zeros(0, np.longdouble)
    top = float(ang.max()) if ang.size else 0.0
    print(f"{what}: {int(mask.sum())} trigonometric-path normals compared, {left_out} left out by the gap rule, "
          f"largest angle {top:.3g} rad, limit {limit:.3g} rad (reference vs long double {worst:.3g})")
    assert top <= limit
    if not exempt:
        assert left_out <= 0.05 * len(got)
    n2 = (got[~det] ** 2).sum(axis=1)
    assert (np.abs(n2 - 1.0) < 1e-12).all()


@pytest.mark.parametrize("name", sorted(NC.cases()))
def test_normals_and_covariances(pkg, gpu, name):
    pts, k, radius, prior = NC.cases()[name]
    ref = NC.reference(name)
    p, nrm, cov = _estimate(pkg, name)
    assert cov.shape == (len(pts), 3, 3) and nrm.shape == (len(pts), 3)
    assert_bitwise(cov, ref["cov"], f"{name}: covariances")
    _compare_normals(nrm, ref, name, exempt=name in NC.EXEMPT_FROM_GAP_RULE)
    if prior is not None:  # the prior decides the sign wherever the dot product is not marginal
        d_ref = (ref["normals"] * prior).sum(axis=1)
        sure = np.abs(d_ref) > 1e-6
        assert ((nrm * prior).sum(axis=1)[sure] > 0).all()
    # the covariance calls alone: the same matrices, and no normals appear
    q = _pcd(pkg, pts)
    assert q.estimate_covariances(_param(pkg, k, radius)) is None
    assert q.has_covariances() and not q.has_normals()
    assert_bitwise(np.array(q.covariances), ref["cov"], f"{name}: estimate_covariances")
    r = _pcd(pkg, pts)
    st = pkg.geometry.PointCloud.estimate_point_covariances(r, _param(pkg, k, radius))
    assert not r.has_covariances()
    assert_bitwise(np.asarray(st), ref["cov"], f"{name}: estimate_point_covariances")


def test_default_search_param_is_knn_30(pkg, gpu):
    pts = NC.cases()["box_k30"][0]
    ref = NC.reference("box_k30")
    p = _pcd(pkg, pts)
    p.estimate_normals()
    assert_bitwise(np.array(p.covariances), ref["cov"], "estimate_normals() covariances")
    q = _pcd(pkg, pts)
    q.estimate_covariances()
    assert_bitwise(np.array(q.covariances), ref["cov"], "estimate_covariances() covariances")


def test_repeat_run_is_bit_identical(pkg, gpu):
    for name in ("box_k30", "lattice_k16", "far_point_k30"):
        _, n1, c1 = _estimate(pkg, name)
        _, n2, c2 = _estimate(pkg, name)
        assert_bitwise(n1, n2, f"{name}: normals of two runs")
        assert_bitwise(c1, c2, f"{name}: covariances of two runs")


def test_estimating_twice_keeps_the_orientation(pkg, gpu):
    """the second call takes the first call's normals as priors: the same lines, and no sign may turn"""
    p, first, _ = _estimate(pkg, "box_k30")
    p.orient_normals_to_align_with_direction((0.3, -0.5, 0.8))
    oriented = np.array(p.normals)
    p.estimate_normals(pkg.geometry.KDTreeSearchParamKNN(30))
    assert_bitwise(np.array(p.normals), oriented, "estimate_normals over its own oriented result")
    assert (np.abs(oriented) == np.abs(first)).all()


def _orientation_inputs():
    ref = NC.reference("box_k30")
    pts = NC.cases()["box_k30"][0]
    N = ref["normals"].copy()
    N[[0, 7, 300]] = 0.0  # zero normals take the reference vector
    return pts, N


def test_orient_to_direction_bitwise(pkg, gpu):
    pts, N = _orientation_inputs()
    for d in ((0.0, 0.0, 1.0), (0.3, -0.5, 0.8), (-1.0, 0.0, 0.0)):
        p = _pcd(pkg, pts, N)
        assert p.orient_normals_to_align_with_direction(d) is None
        assert_bitwise(np.array(p.normals), NR.orient_to_direction(N, d), f"orient to direction {d}")
    p = _pcd(pkg, pts, N)
    p.orient_normals_to_align_with_direction()
    assert_bitwise(np.array(p.normals), NR.orient_to_direction(N, (0.0, 0.0, 1.0)), "default direction +z")


def test_orient_towards_camera_bitwise(pkg, gpu):
    pts, N = _orientation_inputs()
    for cam in ((0.0, 0.0, 0.0), (1.0, -2.0, 3.0), tuple(pts[7])):  # the last one sits on a zero-normal point
        p = _pcd(pkg, pts, N)
        assert p.orient_normals_towards_camera_location(cam) is None
        assert_bitwise(np.array(p.normals), NR.orient_to_camera(N, pts, cam), f"orient towards camera {cam}")
    assert NR.orient_to_camera(N, pts, tuple(pts[7]))[7].tolist() == [0.0, 0.0, 1.0]
    p = _pcd(pkg, pts, N)
    p.orient_normals_towards_camera_location()
    assert_bitwise(np.array(p.normals), NR.orient_to_camera(N, pts, (0.0, 0.0, 0.0)), "default camera at the origin")


def test_normalize_normals_bitwise(pkg, gpu):
    pts, N = _orientation_inputs()
    rng = np.random.default_rng(21)
    M = N * rng.uniform(0.01, 100.0, (len(N), 1)) + rng.normal(0, 0.1, N.shape) * (N != 0).any(axis=1)[:, None]
    p = _pcd(pkg, pts, M)
    assert p.normalize_normals() is p
    assert_bitwise(np.array(p.normals), NR.normalize(M), "normalize_normals")
    assert (np.array(p.normals)[[0, 7, 300]] == 0).all()


def test_signs_after_orienting_the_gpu_normals(pkg, gpu):
    pts = NC.cases()["box_k30"][0]
    ref = NC.reference("box_k30")
    cam = np.array([1.0, -2.3, 1.5])
    p, _, _ = _estimate(pkg, "box_k30")
    p.orient_normals_towards_camera_location(cam)
    got = np.array(p.normals)
    want = NR.orient_to_camera(ref["normals"], pts, cam)
    v = cam - pts
    sure = np.abs((want * v).sum(axis=1)) > 1e-6 * np.linalg.norm(v, axis=1)
    assert sure.sum() > 1400
    assert (np.sign((got * want).sum(axis=1))[sure] > 0).all()
    assert ((got * v).sum(axis=1)[sure] > 0).all()


def test_device_resident_cloud_from_voxel_down_sample(pkg, synth, seq16, gpu):
    """one frame of the package's own pipeline, never downloaded before the normals are estimated"""
    depth, color, ext = seq16
    intr = pkg.camera.PinholeCameraIntrinsic(*ref_intr(synth))
    rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(color[0]), pkg.geometry.Image(depth[0]), depth_scale=1000.0, depth_trunc=5.0,
        convert_rgb_to_intensity=False)
    ds = pkg.geometry.PointCloud.create_from_rgbd_image(rgbd, intr, ext[0]).voxel_down_sample(0.08)
    assert ds._xyz._h is None  # still on the device only
    ds.estimate_normals(pkg.geometry.KDTreeSearchParamHybrid(0.3, 20))
    assert ds._xyz._h is None and ds._nrm._h is None and ds._cov._h is None
    ds.orient_normals_towards_camera_location(np.linalg.inv(ext[0])[:3, 3])
    pts = np.array(ds.points)
    print(f"surface cloud after voxel_down_sample(0.08): {len(pts)} points")
    assert 200 < len(pts) <= 5000
    ref = NR.estimate(pts, 20, 0.3, None, longdouble=True)
    assert_bitwise(np.array(ds.covariances), ref["cov"], "surface cloud covariances")
    _compare_normals(np.array(ds.normals), ref, "surface cloud")
    sub = ds.select_by_index(list(range(0, len(pts), 2)))  # normals are carried through
    assert_bitwise(np.array(sub.normals), np.array(ds.normals)[::2], "select_by_index carries the normals")


def test_grid_refusal_leaves_no_state(pkg, gpu):
    _, before, cov_before = _estimate(pkg, "n257_k30")
    pts = NC.cases()["n257_k30"][0].copy()
    for bad in (np.inf, -np.inf):
        q = pts.copy()
        q[100, 1] = bad
        p = _pcd(pkg, q)
        with pytest.raises(RuntimeError, match=r"neighbour grid out of range"):
            p.estimate_normals(pkg.geometry.KDTreeSearchParamKNN(30))
        with pytest.raises(RuntimeError, match=r"neighbour grid out of range"):
            p.estimate_covariances(pkg.geometry.KDTreeSearchParamHybrid(0.1, 30))
        assert not p.has_normals() and not p.has_covariances()
    _, after, cov_after = _estimate(pkg, "n257_k30")
    assert_bitwise(after, before, "same cloud, same normals after the refusal")
    assert_bitwise(cov_after, cov_before, "same cloud, same covariances after the refusal")
