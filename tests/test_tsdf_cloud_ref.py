"""The numpy restatement of ExtractPointCloud / ExtractVoxelPointCloud (tests/tsdf_cloud_ref.py, DESIGN.md §4 A.9,
A.10) checked against geometry it cannot know: a sphere's radius and outward direction, a slab's exact faces, and
the canonical order.  No GPU."""
import numpy as np
import pytest

import tsdf_cloud_ref as R


@pytest.fixture(scope="module")
def sphere():
    keys, tsdf, weight, color = R.sphere_units()
    stats = {}
    out = R.extract_point_cloud(keys, tsdf, weight, color, R.SPHERE_VL, stats=stats)
    return (keys, tsdf, weight, color), out, stats


def test_sphere_fixture_counts(sphere):
    (keys, tsdf, weight, color), out, stats = sphere
    assert keys.shape == (7, 3) and tsdf.shape == (7, 4096)
    assert len(out["points"]) == 1800
    assert out["normals"].shape == (1800, 3) and out["colors"].shape == (1800, 3)
    vp, vc = R.extract_voxel_point_cloud(keys, tsdf, weight, R.SPHERE_VL)
    assert len(vp) == 9840 and vc.shape == (9840, 3)
    assert np.all(vc[:, 0] == vc[:, 1]) and np.all(vc[:, 0] == vc[:, 2])
    assert vc.min() >= 0.0 and vc.max() < 1.0
    # the paths the fixture is made to take: edges and trilinear corners that cross into other units, present and
    # missing, and normal samples inside the missing unit; the clamp is reachable by rounding only
    assert stats == {"edges_leaving": 1422, "edges_into_missing": 269, "missing_samples": 24,
                     "missing_corners": 892, "wrapped_corners": 5512, "clamped": 0}


def test_sphere_points_lie_on_the_sphere(sphere):
    """A chord of length h = 0.01 on a sphere of R = 0.105 leaves it by at most h^2 / (8 R) = 1.19e-4; 1.25e-4 allows
    for the float32 tsdf."""
    _, out, _ = sphere
    d = out["points"] - np.array(R.SPHERE_CENTRE)
    err = np.abs(np.linalg.norm(d, axis=1) - R.SPHERE_R).max()
    print("max |r - R| =", err)
    assert err <= 1.25e-4


def test_sphere_normals_point_outwards(sphere):
    _, out, _ = sphere
    d = out["points"] - np.array(R.SPHERE_CENTRE)
    n = out["normals"]
    assert np.all(np.sum(n * n, axis=1) > 0)  # no zero-length normal
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-15)
    cos = np.sum(n * d, axis=1) / np.linalg.norm(d, axis=1)
    print("min cos =", cos.min())
    assert cos.min() > 0.99


def test_sphere_colours_interpolate_the_voxel_colours(sphere):
    (keys, tsdf, weight, color), out, _ = sphere
    assert out["colors"].min() >= 0.0 and out["colors"].max() <= 1.0
    none = R.extract_point_cloud(keys, tsdf, weight, None, R.SPHERE_VL)
    assert none["colors"] is None
    np.testing.assert_array_equal(none["points"], out["points"])
    np.testing.assert_array_equal(none["normals"], out["normals"])
    # a float32 colour input is used as it is: the same as narrowing the float64 one
    f32 = R.extract_point_cloud(keys, tsdf, weight, color.astype(np.float32), R.SPHERE_VL)
    np.testing.assert_array_equal(f32["colors"], out["colors"])


def test_slab_faces_are_exact():
    """Every value of the slab is dyadic, so A.9 is exact on it: the points sit on the two faces (to within float32
    rounding of tsdf, here none) and the normals are exactly (0, 0, -1) below and (0, 0, +1) above."""
    keys, tsdf, weight, color = R.slab_units()
    out = R.extract_point_cloud(keys, tsdf, weight, color, R.SLAB_VL)
    p, n, e = out["points"], out["normals"], out["edge"]
    assert len(p) == 4 * 256 * 2 and out["colors"] is None
    assert np.all(e[:, 4] == 2)
    low = (e[:, 3] & 15) == 3
    assert low.sum() == 4 * 256 and np.all((e[~low, 3] & 15) == 11)
    zl, zh = (R.SLAB_LOW + 0.5) * R.SLAB_VL, (R.SLAB_HIGH + 0.5) * R.SLAB_VL
    tol = 2.0 ** -24 * R.SLAB_VL  # float32 rounding of a tsdf of either end moves the point by less than this
    assert np.abs(p[low, 2] - zl).max() <= tol and np.abs(p[~low, 2] - zh).max() <= tol
    assert np.all(n[low] == np.array([0.0, 0.0, -1.0]))
    assert np.all(n[~low] == np.array([0.0, 0.0, 1.0]))
    # x and y are voxel centres
    g = p[:, :2] / R.SLAB_VL - 0.5
    assert np.all(g == np.round(g)) and g.min() == -16 and g.max() == 15


def test_canonical_order(sphere):
    """Unit key, then voxel x*256 + y*16 + z, then axis, whatever order the units come in."""
    (keys, tsdf, weight, color), out, _ = sphere
    e = out["edge"]
    assert np.all((e[:, :3] >= -1) & (e[:, :3] <= 0)) and e[:, 3].max() < 4096 and set(e[:, 4]) == {0, 1, 2}
    rank = (((e[:, 0] + 1) * 2 + (e[:, 1] + 1)) * 2 + (e[:, 2] + 1)) * (4096 * 3) + e[:, 3] * 3 + e[:, 4]
    assert np.all(np.diff(rank) > 0)
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    again = R.extract_point_cloud(keys[perm], tsdf[perm], weight[perm], color[perm], R.SPHERE_VL)
    for k in ("points", "colors", "normals", "edge"):
        np.testing.assert_array_equal(again[k], out[k])
    vp, vc = R.extract_voxel_point_cloud(keys, tsdf, weight, R.SPHERE_VL)
    vp2, vc2 = R.extract_voxel_point_cloud(keys[perm], tsdf[perm], weight[perm], R.SPHERE_VL)
    np.testing.assert_array_equal(vp2, vp)
    np.testing.assert_array_equal(vc2, vc)
    # the voxel cloud walks units by key and voxels by index too: its first point is unit (-1, -1, -1)'s first usable
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    first = np.flatnonzero(R.usable(tsdf[order[0]], weight[order[0]]))[0]
    idx = np.array([first >> 8, (first >> 4) & 15, first & 15])
    np.testing.assert_array_equal(vp[0], R._centres(keys[order[0]].astype(np.int64), idx, R.SPHERE_VL))


def test_normals_of_a_subset(sphere):
    (keys, tsdf, weight, color), out, _ = sphere
    sel = np.arange(0, 1800, 37)
    sub = R.extract_point_cloud(keys, tsdf, weight, color, R.SPHERE_VL, normals_at=sel)
    np.testing.assert_array_equal(sub["normals"], out["normals"][sel])
    np.testing.assert_array_equal(sub["points"], out["points"])
