"""GPU parity of PointCloud.cluster_dbscan (csrc/cluster.hip over the grid of csrc/grid.h) against the exhaustive float64
reference of tests/dbscan_ref.py: the labels, bit for bit as int32.  Every cloud has at most 5 000 points; the
designed clouds are those of tests/dbscan_clouds.py, whose properties test_dbscan_api.py asserts on the CPU."""
import numpy as np
import pytest

import dbscan_clouds as DC
import dbscan_ref as DB
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu


def _pcd(pkg, pts):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.ascontiguousarray(pts, np.float64))
    return p


def _gpu(pkg, pts, eps, mp):
    out = _pcd(pkg, pts).cluster_dbscan(eps, mp)
    assert isinstance(out, pkg.utility.IntVector) and len(out) == len(pts)
    assert all(type(v) is int for v in out[:16])
    return np.asarray(out, np.int32)


def _check(pkg, pts, eps, mp, what):
    assert len(pts) <= 5000
    ref = DB.cluster_dbscan(pts, eps, mp)
    assert_bitwise(_gpu(pkg, pts, eps, mp), ref, what)
    return ref


def test_dbscan_random_blobs(pkg, gpu):
    rng = np.random.default_rng(51)
    for pts, eps, mp in DC.random_cases(2):
        _check(pkg, pts, eps, mp, f"DBSCAN({eps}, {mp}) blobs and noise")
        _check(pkg, pts[rng.permutation(len(pts))], eps, mp, f"DBSCAN({eps}, {mp}) blobs and noise, permuted")


def test_dbscan_contested_border_points(pkg, gpu):
    pts, eps, mp, single = DC.contested()
    ref = _check(pkg, pts, eps, mp, "DBSCAN contested border points")
    assert len(single) >= 5 and (ref[single] == 0).all() and ref.max() == 1


def test_dbscan_noise_first_and_isolated(pkg, gpu):
    pts, eps, mp, n_fringe, n_lone = DC.noise_first()
    ref = _check(pkg, pts, eps, mp, "DBSCAN border points stored before their cluster")
    assert (ref[:n_fringe] >= 0).all() and (ref[len(pts) - n_lone:] == -1).all()


def test_dbscan_lattice_at_exactly_eps(pkg, gpu):
    for name, pts, eps, mp in DC.lattice_cases():
        _check(pkg, pts, eps, mp, f"DBSCAN lattice {name}, min_points = {mp}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_dbscan_cell_straddle(pkg, gpu, axis):
    """pairs closer than eps whose cells in a grid of cell size exactly eps differ by 2 (tests/test_gpu_ror_edges.py):
    each is a two-point cluster for min_points = 2, numbered in pair order"""
    ran = 0
    for pts, r, k in DC.straddle_cases(axis):
        ref = _check(pkg, pts, r, 2, f"DBSCAN straddling pairs along axis {axis} (r = {r})")
        assert ref[1:2 * k + 1].tolist() == np.repeat(np.arange(k), 2).tolist()
        ran += k
    assert ran > 2000


@pytest.mark.parametrize("mp", [2, 3])
def test_dbscan_chain(pkg, gpu, mp):
    """no iteration cap: 4 096 points, each a neighbour of the next only, are one cluster in any index order"""
    pts = DC.chain(4096)
    rng = np.random.default_rng(53)
    for name, p in (("index order", pts), ("reversed", pts[::-1]), ("permuted", pts[rng.permutation(4096)])):
        ref = _check(pkg, p, DC.CHAIN_EPS, mp, f"DBSCAN chain of 4096, {name}, min_points = {mp}")
        assert (ref == 0).all()
    two = DC.two_chains()
    ref = _check(pkg, two, DC.CHAIN_EPS, mp, f"DBSCAN two interleaved chains, min_points = {mp}")
    assert (ref[0::2] == 0).all() and (ref[1::2] == 1).all()


def test_dbscan_coincident_points(pkg, gpu):
    pts, eps, m, sizes, gid = DC.coincident()
    ref = _check(pkg, pts, eps, m, "DBSCAN coincident groups")
    assert ((ref >= 0) == (sizes >= m)).all()


def test_dbscan_small_and_odd_sizes(pkg, gpu):
    for name, pts, eps, mp in DC.small_cases():
        _check(pkg, pts, eps, mp, f"DBSCAN {name}, min_points = {mp}")


def test_dbscan_surface_cloud(pkg, synth, seq16, gpu):
    """one frame of the package's own pipeline: create_from_rgbd_image, then voxel_down_sample"""
    depth, color, ext = seq16
    intr = pkg.camera.PinholeCameraIntrinsic(*ref_intr(synth))
    rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(color[0]), pkg.geometry.Image(depth[0]), depth_scale=1000.0, depth_trunc=5.0,
        convert_rgb_to_intensity=False)
    cloud = pkg.geometry.PointCloud.create_from_rgbd_image(rgbd, intr, ext[0])
    voxel = 0.05
    ds = cloud.voxel_down_sample(voxel)
    pts = np.asarray(ds.points).reshape(-1, 3)
    print(f"surface cloud: {len(cloud.points)} points, {len(pts)} after voxel_down_sample({voxel})")
    assert 500 < len(pts) <= 5000
    for eps, mp in ((0.055, 3), (0.07, 6), (0.08, 8)):
        ref = DB.cluster_dbscan(pts, eps, mp)
        assert_bitwise(np.asarray(ds.cluster_dbscan(eps, mp), np.int32), ref, f"DBSCAN({eps}, {mp}) surface cloud")
        print(f"  eps = {eps}, min_points = {mp}: {ref.max() + 1} clusters, {(ref == -1).sum()} noise points")


def test_dbscan_grid_refusal_leaves_no_state(pkg, gpu):
    eps = 0.01
    cloud = np.random.default_rng(55).normal(0, 0.03, (1000, 3))
    before = _check(pkg, cloud, eps, 5, "DBSCAN before the refusal")
    far = np.array([[0.0, 0.0, 0.0], [2.0e6 * eps, 0.0, 0.0]])
    with pytest.raises(RuntimeError, match=r"neighbour grid out of range \(radius too small for the extent\)"):
        _gpu(pkg, far, eps, 1)
    with pytest.raises(RuntimeError, match=r"neighbour grid out of range \(radius too small for the extent\)"):
        _gpu(pkg, far[:, [2, 1, 0]], eps, 1)
    after = _check(pkg, cloud, eps, 5, "DBSCAN after the refusal")
    assert_bitwise(after, before, "same cloud, same answer")
    assert before.max() >= 0 and (before == -1).any()


def test_dbscan_is_deterministic(pkg, gpu):
    pts = DC.blob_cloud(57, 500)
    big = np.concatenate([pts + [2.0 * a, 0.0, 0.0] for a in range(10)])  # 5 000 points
    a = _gpu(pkg, big, 0.08, 5)
    b = _gpu(pkg, big, 0.08, 5)
    assert_bitwise(a, b, "the same cloud twice")
    assert_bitwise(a, DB.cluster_dbscan(big, 0.08, 5), "DBSCAN(0.08, 5) on 5 000 points")
