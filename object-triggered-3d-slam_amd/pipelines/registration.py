"""open3d.pipelines.registration counterpart: point-to-point ICP and evaluate_registration on the GPU
(eval_cone.py:89-97, eval_table_chair.py:90-104, eval_cardboard.py:88-96), and the two calls a global registration
stands on: compute_fpfh_feature and correspondences_from_features.

Every call goes through the C ABI (ot_registration_icp / ot_evaluate_registration, csrc/icp.hip: the nearest-neighbour
search, the reductions, the rigid fit and the iteration loop all run on the device; ot_compute_fpfh_feature /
ot_correspondences_from_features, csrc/features.hip).  The definitions built against and the canonical order of the
correspondence set are in DESIGN.md §4 ("registration", "features").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _device as D
from .. import _lib as L
from ..geometry import _search_args
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


# ------------------------------------------------------------------------------------------------ features
class Feature:
    """open3d.pipelines.registration.Feature: `data` is a float64 (dim, num) array, one column per point.  The device
    copy is point-major (num, dim), the layout the kernels read and write; either copy is made from the other when it
    is first asked for."""

    def __init__(self):
        self._h = np.zeros((0, 0))  # (dim, num), or None while only the device copy exists
        self._d = None              # (num, dim) device tensor, or None

    @classmethod
    def _from_dev(cls, t):
        f = cls()
        f._h, f._d = None, t
        return f

    @property
    def data(self):
        """The host array itself (a view, as Open3D's): edits made through it are seen, so the device copy is dropped
        and made again from the host copy at the next GPU use."""
        if self._h is None:
            self._h = np.ascontiguousarray(D.to_host(self._d).T)
        self._d = None
        return self._h

    @data.setter
    def data(self, v):
        a = np.array(v, dtype=np.float64, copy=True, order="C")
        if a.ndim != 2:
            raise RuntimeError(f"Feature.data expects a (dim, num) array, got {a.shape}")
        self._h, self._d = a, None

    def _dev(self):
        if self._d is None:
            self._d = D.to_device(np.ascontiguousarray(self._h.T))
        return self._d

    def dimension(self):
        return int(self._h.shape[0] if self._h is not None else self._d.shape[1])

    def num(self):
        return int(self._h.shape[1] if self._h is not None else self._d.shape[0])

    def resize(self, dim, n):
        self._h, self._d = np.zeros((int(dim), int(n))), None

    def select_by_index(self, indices, invert=False):
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if invert:
            mask = np.ones(self.num(), bool)
            mask[idx] = False
            idx = np.nonzero(mask)[0]
        out = Feature()
        out._h = np.ascontiguousarray(self.data[:, idx])
        return out

    def __repr__(self):
        return (f"Feature class with dimension = {self.dimension()} and num = {self.num()}\n"
                "Access its data via data member.")


def compute_fpfh_feature(input, search_param):
    """open3d.pipelines.registration.compute_fpfh_feature — ot_compute_fpfh_feature: the 33-bin FPFH of every point
    over its first knn / max_nn (1..128) neighbours by (distance, index), hybrid: those inside the radius
    (DESIGN.md §4 "features").  The cloud needs normals; KDTreeSearchParamRadius is refused.  A device-resident cloud
    is read where it is and the feature stays on the device until `data` is read."""
    if not input.has_normals():
        raise RuntimeError("[ComputeFPFHFeature] Failed because input point cloud has no normal.")
    knn, radius = _search_args("ComputeFPFHFeature", search_param, limit=128,
                               what="the histogram is a distance-ordered sum")
    n = len(input._xyz)
    if len(input._nrm) != n:
        raise RuntimeError(f"[ComputeFPFHFeature] {len(input._nrm)} normals for {n} points")
    out = D.empty((n, 33), "float64")
    L.call("ot_compute_fpfh_feature", D.ptr(input._xyz.dev()), D.ptr(input._nrm.dev()), n, knn, radius, D.ptr(out),
           None, D.stream_ptr())
    return Feature._from_dev(out)


def correspondences_from_features(source_features, target_features, mutual_filter=False,
                                  mutual_consistency_ratio=0.1):
    """open3d.pipelines.registration.correspondences_from_features — ot_correspondences_from_features: per source
    column the target column with the smallest (squared distance, index); with mutual_filter only the pairs the
    reverse match agrees with, unless fewer than mutual_consistency_ratio * num are left, in which case all pairs are
    returned.  Returns a Vector2iVector of (source index, target index) in ascending source index."""
    dim, n, m = source_features.dimension(), source_features.num(), target_features.num()
    if target_features.dimension() != dim:
        raise RuntimeError(f"[CorrespondencesFromFeatures] the source features have dimension {dim}, the target "
                           f"features {target_features.dimension()}")
    if n == 0:
        return Vector2iVector()
    if m == 0:
        raise RuntimeError("[CorrespondencesFromFeatures] the target has no features")
    if not 1 <= dim <= 128:
        raise RuntimeError(f"[CorrespondencesFromFeatures] the feature dimension must lie in 1..128, got {dim}")
    corr = D.empty((n, 2), "int32")
    k, fell = C.c_int64(0), C.c_int32(0)
    L.call("ot_correspondences_from_features", D.ptr(source_features._dev()), n, D.ptr(target_features._dev()), m, dim,
           1 if mutual_filter else 0, float(mutual_consistency_ratio), D.ptr(corr), C.byref(k), C.byref(fell),
           D.stream_ptr())
    return Vector2iVector._view(D.to_host(corr[:k.value]))
