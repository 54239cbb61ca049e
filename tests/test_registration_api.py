"""pipelines.registration and the PointCloud motion API without a device: names, defaults, the closed-form rotation,
the three new C-ABI symbols, and the numpy reference the GPU tests are checked against (it must itself recover the
known transformation of the analytic scene)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import icp_ref as R


def test_criteria_defaults_and_argument_names(pkg):
    reg = pkg.pipelines.registration
    c = reg.ICPConvergenceCriteria()
    assert (c.relative_fitness, c.relative_rmse, c.max_iteration) == (1e-6, 1e-6, 30)
    c = reg.ICPConvergenceCriteria(max_iteration=2000)  # the evaluation scripts' call
    assert (c.relative_fitness, c.relative_rmse, c.max_iteration) == (1e-6, 1e-6, 2000)
    c = reg.ICPConvergenceCriteria(relative_fitness=1e-3, relative_rmse=1e-4, max_iteration=7)
    assert (c.relative_fitness, c.relative_rmse, c.max_iteration) == (1e-3, 1e-4, 7)
    assert list(inspect.signature(reg.registration_icp).parameters) == [
        "source", "target", "max_correspondence_distance", "init", "estimation_method", "criteria"]
    assert list(inspect.signature(reg.evaluate_registration).parameters) == [
        "source", "target", "max_correspondence_distance", "transformation"]


def test_estimation_and_result_classes(pkg):
    reg = pkg.pipelines.registration
    assert reg.TransformationEstimationPointToPoint().with_scaling is False
    assert reg.TransformationEstimationPointToPoint(with_scaling=False).with_scaling is False
    with pytest.raises(RuntimeError, match="not supported"):
        reg.TransformationEstimationPointToPoint(with_scaling=True)
    res = reg.RegistrationResult()
    assert res.transformation.shape == (4, 4) and res.transformation.dtype == np.float64
    assert np.array_equal(res.transformation, np.eye(4))
    assert (res.fitness, res.inlier_rmse, res.iterations) == (0.0, 0.0, 0)
    corr = np.asarray(res.correspondence_set)
    assert corr.shape == (0, 2) and corr.dtype == np.int32


def test_point_cloud_has_the_motion_api(pkg):
    for name in ("transform", "rotate", "translate", "get_center", "__deepcopy__"):
        assert callable(getattr(pkg.geometry.PointCloud, name)), name
    assert np.array_equal(pkg.geometry.PointCloud().get_center(), np.zeros(3))
    ev = __import__("importlib").import_module(pkg.__name__ + ".evaluation")
    for name in ("apply_transform", "refine_icp", "calculate_metrics"):
        assert callable(getattr(ev, name)), name


@pytest.mark.parametrize("angles", [(0.0, 0.0, 0.0), (0.3, -1.1, 2.0), (np.pi / 2, 0.25, -np.pi / 3),
                                    (-2.9, 1.5, 0.01)])
def test_rotation_matrix_from_xyz_closed_form(pkg, angles):
    Rm = pkg.geometry.get_rotation_matrix_from_xyz(angles)
    assert Rm.shape == (3, 3) and Rm.dtype == np.float64
    assert np.abs(Rm - R.rotation_xyz_closed_form(*angles)).max() <= 4e-16
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15
    a, b, c = angles
    rx = pkg.geometry.get_rotation_matrix_from_xyz((a, 0, 0))
    ry = pkg.geometry.get_rotation_matrix_from_xyz((0, b, 0))
    rz = pkg.geometry.get_rotation_matrix_from_xyz((0, 0, c))
    assert np.abs(Rm - rx @ ry @ rz).max() <= 4e-16


NEW_SYMBOLS = ("ot_transform_points", "ot_evaluate_registration", "ot_registration_icp")


def test_new_symbols_in_header_table_and_library(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(pkg._lib.HEADER_PATH).read(), flags=re.S)
    lib = C.CDLL(pkg._lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in otslam.h"
        assert name in pkg._lib.SIGNATURES, f"{name} not bound"
        assert hasattr(lib, name), f"{name} not exported"
    assert len(pkg._lib.SIGNATURES["ot_registration_icp"]) == 16
    assert len(pkg._lib.SIGNATURES["ot_evaluate_registration"]) == 11
    assert len(pkg._lib.SIGNATURES["ot_transform_points"]) == 7


def test_invalid_distance_is_refused_before_any_device_work(pkg):
    lib = pkg.native_library()
    eye = np.eye(4)
    st = lib.ot_registration_icp(None, 0, None, 0, 0.0, eye.ctypes.data_as(C.c_void_p), 1e-6, 1e-6, 30,
                                 None, None, None, None, None, None, None)
    assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert lib.ot_last_error() == b"Invalid max_correspondence_distance."


@pytest.mark.parametrize("deg", [1, 3])
def test_reference_icp_recovers_the_known_transformation(deg):
    """Pins the checker: on the analytic scene the numpy restatement converges to T_gt."""
    src, tgt, T_gt = R.scene(deg)
    assert src.shape == (2800, 3) and tgt.shape == (4800, 3)
    res = R.reference_icp(deg)
    assert res.iterations < 30
    assert res.fitness == 2500 / 2800
    assert res.inlier_rmse < 1e-12
    assert np.abs(res.transformation - T_gt).max() <= 1e-12
    assert np.array_equal(res.corr[:, 0], np.arange(2500))
