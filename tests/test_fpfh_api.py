"""compute_fpfh_feature / correspondences_from_features without a device: the C ABI declaration and binding, the
Feature container, and every refusal (raised before any device work)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, assert_bitwise

CALLS = (("ot_compute_fpfh_feature", 8), ("ot_correspondences_from_features", 11))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_declares_and_table_binds_the_calls(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.native_library()
    for name, nargs in CALLS:
        assert re.search(r"\bot_status\s+" + name + r"\s*\(", src)
        assert len(pkg._lib.SIGNATURES[name]) == nargs
        assert name not in lib._ot_missing
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "compute_fpfh_feature" in text and "correspondences_from_features" in text


def test_exported_as_open3d_names_them(pkg):
    r = pkg.pipelines.registration
    for name in ("Feature", "compute_fpfh_feature", "correspondences_from_features"):
        assert hasattr(r, name)


# ------------------------------------------------------------------------------------------------ Feature
def test_feature_container(pkg):
    r = pkg.pipelines.registration
    f = r.Feature()
    assert f.dimension() == 0 and f.num() == 0 and f.data.shape == (0, 0)
    f.resize(33, 5)
    assert f.dimension() == 33 and f.num() == 5 and f.data.shape == (33, 5) and f.data.dtype == np.float64
    assert (f.data == 0).all()
    a = np.arange(12.0).reshape(3, 4)
    f.data = a
    assert f.dimension() == 3 and f.num() == 4
    assert_bitwise(f.data, a, "data round trip")
    a[0, 0] = 99.0  # the setter copied
    assert f.data[0, 0] == 0.0
    f.data[2, 3] = -1.0  # the getter hands out the array itself
    assert f.data[2, 3] == -1.0
    f.data = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert f.data.dtype == np.float64
    assert "dimension = 2" in repr(f) and "num = 3" in repr(f)
    with pytest.raises(RuntimeError, match="dim, num"):
        f.data = np.zeros(3)


def test_feature_select_by_index(pkg):
    f = pkg.pipelines.registration.Feature()
    f.data = np.arange(20.0).reshape(4, 5)
    s = f.select_by_index([3, 0, 3])
    assert s.dimension() == 4 and s.num() == 3
    assert_bitwise(s.data, f.data[:, [3, 0, 3]], "selected columns, in the order asked for")
    inv = f.select_by_index([1, 4], invert=True)
    assert_bitwise(inv.data, f.data[:, [0, 2, 3]], "the other columns")
    s.data[0, 0] = -5.0  # a copy
    assert f.data[0, 3] == 3.0
    assert f.select_by_index([]).num() == 0 and f.select_by_index([]).dimension() == 4


# ------------------------------------------------------------------------------------------------ Python refusals
def _cloud(pkg, n=4, normals=True):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.arange(3.0 * n).reshape(n, 3))
    if normals and n:
        p.normals = pkg.utility.Vector3dVector(np.tile([0.0, 0.0, 1.0], (n, 1)))
    return p


def test_compute_fpfh_refusals_need_no_device(pkg):
    g, r = pkg.geometry, pkg.pipelines.registration
    for p in (_cloud(pkg, 4, normals=False), _cloud(pkg, 0)):
        with pytest.raises(RuntimeError) as e:
            r.compute_fpfh_feature(p, g.KDTreeSearchParamKNN(10))
        assert str(e.value) == "[ComputeFPFHFeature] Failed because input point cloud has no normal."
    p = _cloud(pkg)
    with pytest.raises(RuntimeError, match=r"\[ComputeFPFHFeature\] KDTreeSearchParamRadius is not supported.*"
                                           r"at most 128 neighbours; use KDTreeSearchParamHybrid"):
        r.compute_fpfh_feature(p, g.KDTreeSearchParamRadius(0.1))
    for k in (0, -1, 129, 1000):
        with pytest.raises(RuntimeError, match=r"knn must lie in 1\.\.128"):
            r.compute_fpfh_feature(p, g.KDTreeSearchParamKNN(k))
        with pytest.raises(RuntimeError, match=r"max_nn must lie in 1\.\.128"):
            r.compute_fpfh_feature(p, g.KDTreeSearchParamHybrid(0.1, k))
    for rad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="radius > 0"):
            r.compute_fpfh_feature(p, g.KDTreeSearchParamHybrid(rad, 100))
    for bad in (30, None):
        with pytest.raises(RuntimeError, match="search_param must be"):
            r.compute_fpfh_feature(p, bad)


def test_normals_messages_are_untouched(pkg):
    g = pkg.geometry
    p = _cloud(pkg)
    with pytest.raises(RuntimeError) as e:
        p.estimate_normals(g.KDTreeSearchParamRadius(0.1))
    assert str(e.value) == ("[EstimateNormals] KDTreeSearchParamRadius is not supported: its neighbour list is "
                            "unbounded and the covariance is a distance-ordered sum over at most 64 neighbours; use "
                            "KDTreeSearchParamHybrid(radius, max_nn)")
    with pytest.raises(RuntimeError) as e:
        p.estimate_normals(g.KDTreeSearchParamKNN(100))
    assert str(e.value) == "[EstimateNormals] knn must lie in 1..64 (the neighbour list is kept on chip), got 100"


def test_correspondences_refusals_need_no_device(pkg):
    r = pkg.pipelines.registration
    a, b, empty = r.Feature(), r.Feature(), r.Feature()
    a.data, b.data = np.zeros((33, 4)), np.zeros((32, 4))
    with pytest.raises(RuntimeError, match="dimension 33.*32"):
        r.correspondences_from_features(a, b)
    empty.resize(33, 0)
    with pytest.raises(RuntimeError, match="the target has no features"):
        r.correspondences_from_features(a, empty, mutual_filter=True)
    out = r.correspondences_from_features(empty, a)  # an empty source: no pairs, no device
    assert isinstance(out, pkg.utility.Vector2iVector) and len(out) == 0
    wide = r.Feature()
    wide.resize(129, 2)
    with pytest.raises(RuntimeError, match=r"1\.\.128"):
        r.correspondences_from_features(wide, wide)


# ------------------------------------------------------------------------------------------------ C ABI refusals
@pytest.mark.parametrize("knn,radius,text", [(0, 0.0, "1..128"), (129, 0.0, "1..128"), (-3, 0.1, "1..128"),
                                             (100, float("nan"), "radius is NaN")])
def test_fpfh_argument_errors_need_no_device(pkg, knn, radius, text):
    lib = pkg.native_library()
    pts, out = np.zeros((4, 3)), np.zeros((4, 33))
    st = lib.ot_compute_fpfh_feature(_p(pts), _p(pts), 4, knn, radius, _p(out), None, None)
    assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
    msg = lib.ot_last_error().decode()
    assert msg.startswith("[ComputeFPFHFeature]") and text in msg


def test_fpfh_buffers_and_empty(pkg):
    lib = pkg.native_library()
    pts, out = np.zeros((4, 3)), np.zeros((4, 33))
    assert lib.ot_compute_fpfh_feature(None, None, 0, 100, 0.0, None, None, None) == pkg._lib.OT_OK
    for args in ((None, _p(pts), 4, _p(out)), (_p(pts), None, 4, _p(out)), (_p(pts), _p(pts), 4, None),
                 (_p(pts), _p(pts), 2 ** 31, _p(out))):
        st = lib.ot_compute_fpfh_feature(args[0], args[1], args[2], 30, 0.0, args[3], None, None)
        assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
        assert lib.ot_last_error().decode() == "[ComputeFPFHFeature] invalid buffers"


def test_correspondences_argument_errors_need_no_device(pkg):
    lib = pkg.native_library()
    INV = pkg._lib.OT_ERR_INVALID_ARGUMENT
    f, corr = np.zeros((4, 33)), np.zeros((4, 2), np.int32)
    k, fell = C.c_int64(7), C.c_int32(7)

    def call(src, n, tgt, m, dim, out=_p(corr), kp=C.byref(k)):
        return lib.ot_correspondences_from_features(src, n, tgt, m, dim, 1, 0.1, out, kp, C.byref(fell), None)

    for dim in (0, -1, 129):
        assert call(_p(f), 4, _p(f), 4, dim) == INV
        assert "1..128" in lib.ot_last_error().decode()
    assert call(None, 0, _p(f), 4, 33) == pkg._lib.OT_OK and k.value == 0 and fell.value == 0  # no source: no pairs
    assert call(None, 0, None, 0, 33) == pkg._lib.OT_OK
    assert call(_p(f), 4, None, 0, 33) == INV
    assert lib.ot_last_error().decode() == "[CorrespondencesFromFeatures] the target has no features"
    for args in ((None, 4, _p(f), 4), (_p(f), 4, None, 4), (_p(f), 2 ** 31, _p(f), 4), (_p(f), 4, _p(f), 2 ** 31)):
        assert call(*args, 33) == INV
        assert lib.ot_last_error().decode() == "[CorrespondencesFromFeatures] invalid buffers"
    assert call(_p(f), 4, _p(f), 4, 33, out=None) == INV
    assert call(_p(f), 4, _p(f), 4, 33, kp=None) == INV
    assert lib.ot_last_error().decode().startswith("[CorrespondencesFromFeatures]")
