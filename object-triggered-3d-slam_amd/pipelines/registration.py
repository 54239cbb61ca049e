"""open3d.pipelines.registration counterpart: point-to-point ICP and evaluate_registration on the GPU
(eval_cone.py:89-97, eval_table_chair.py:90-104, eval_cardboard.py:88-96).

Both calls go through the C ABI (ot_registration_icp / ot_evaluate_registration, csrc/icp.hip): the nearest-neighbour
search, the reductions, the rigid fit and the iteration loop all run on the device.  The definition built against and
the canonical order of the correspondence set are in DESIGN.md §4 ("registration").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _lib as L
from ..utility import Vector2iVector


class ICPConvergenceCriteria:
    """open3d.pipelines.registration.ICPConvergenceCriteria."""

    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)

    def __repr__(self):
        return (f"ICPConvergenceCriteria(relative_fitness={self.relative_fitness:e}, "
                f"relative_rmse={self.relative_rmse:e}, max_iteration={self.max_iteration})")


class TransformationEstimationPointToPoint:
    """open3d.pipelines.registration.TransformationEstimationPointToPoint (Eigen::umeyama without scaling)."""

    def __init__(self, with_scaling=False):
        if with_scaling:
            raise RuntimeError("TransformationEstimationPointToPoint(with_scaling=True) is not supported by this "
                               "build (the reference never asks for it)")
        self.with_scaling = False

    def __repr__(self):
        return "TransformationEstimationPointToPoint without scaling."


class RegistrationResult:
    """open3d.pipelines.registration.RegistrationResult, plus `iterations` (fits performed; Open3D does not report
    it)."""

    def __init__(self):
        self.transformation = np.eye(4)
        self.fitness = 0.0
        self.inlier_rmse = 0.0
        self.correspondence_set = Vector2iVector()
        self.iterations = 0

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, and "
                f"correspondence_set size of {len(self.correspondence_set)}\nAccess transformation to get result.")


def _mat4(m, what):
    T = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    if T.shape != (4, 4):
        raise RuntimeError(f"[{what}] expected a 4x4 matrix, got {T.shape}")
    return T


def _clouds(source, target):
    n, m = len(source._xyz), len(target._xyz)
    return n, m, (D.ptr(source._xyz.dev()) if n else None), (D.ptr(target._xyz.dev()) if m else None)


def _finish(res, T, fit, rmse, corr, k, iterations):
    res.transformation = T
    res.fitness, res.inlier_rmse, res.iterations = fit.value, rmse.value, iterations
    if corr is not None and k.value > 0:
        res.correspondence_set = Vector2iVector._view(D.to_host(corr[:k.value]))
    return res


def evaluate_registration(source, target, max_correspondence_distance, transformation=None):
    """open3d.pipelines.registration.evaluate_registration — ot_evaluate_registration."""
    T = _mat4(np.eye(4) if transformation is None else transformation, "EvaluateRegistration")
    n, m, ps, pt = _clouds(source, target)
    corr = D.empty((n, 2), "int32") if n and m else None
    fit, rmse, k = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    L.call("ot_evaluate_registration", ps, n, pt, m, float(max_correspondence_distance), T.ctypes.data_as(C.c_void_p),
           C.byref(fit), C.byref(rmse), D.ptr(corr), C.byref(k), D.stream_ptr() if n and m else None)
    return _finish(RegistrationResult(), T.copy(), fit, rmse, corr, k, 0)


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """open3d.pipelines.registration.registration_icp (eval_cone.py:91-95) — ot_registration_icp.  Point-to-point
    estimation only."""
    T0 = _mat4(np.eye(4) if init is None else init, "RegistrationICP")
    est = TransformationEstimationPointToPoint() if estimation_method is None else estimation_method
    if not isinstance(est, TransformationEstimationPointToPoint):
        raise RuntimeError("[RegistrationICP] only TransformationEstimationPointToPoint is supported by this build")
    crit = ICPConvergenceCriteria() if criteria is None else criteria
    n, m, ps, pt = _clouds(source, target)
    corr = D.empty((n, 2), "int32") if n and m else None
    fit, rmse, k, it = C.c_double(0.0), C.c_double(0.0), C.c_int64(0), C.c_int32(0)
    T = np.zeros((4, 4))
    L.call("ot_registration_icp", ps, n, pt, m, float(max_correspondence_distance), T0.ctypes.data_as(C.c_void_p),
           float(crit.relative_fitness), float(crit.relative_rmse), int(crit.max_iteration),
           T.ctypes.data_as(C.c_void_p), C.byref(fit), C.byref(rmse), D.ptr(corr), C.byref(k), C.byref(it),
           D.stream_ptr() if n and m else None)
    return _finish(RegistrationResult(), T, fit, rmse, corr, k, it.value)
