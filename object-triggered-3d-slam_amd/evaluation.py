"""Restated helpers of the reference's evaluation scripts (eval/eval_cone/eval_cone.py and its table/chair and
cardboard siblings), running on this package.

Each function keeps the reference's Open3D call sequence and constants but takes the Open3D-shaped module as a
parameter (`o3d`, default: this package), as reconstruct.py does.

  apply_transform    <- eval_cone.py:81-87
  refine_icp         <- eval_cone.py:89-97
  calculate_metrics  <- eval_cone.py:99-110
"""
from __future__ import annotations

import copy
import importlib

import numpy as np

ICP_MAX_CORRESPONDENCE_DISTANCE = 0.05  # eval_cone.py:92
ICP_MAX_ITERATION = 2000                # eval_cone.py:94


def _default_o3d():
    return importlib.import_module(__package__)


def apply_transform(pcd, rot, trans, o3d=None):
    """A copy of pcd rotated by the XYZ Euler angles `rot` (degrees) about the origin, then translated by `trans`."""
    o3d = o3d or _default_o3d()
    rx, ry, rz = np.radians(rot[0]), np.radians(rot[1]), np.radians(rot[2])
    R = o3d.geometry.get_rotation_matrix_from_xyz((rx, ry, rz))
    pcd_copy = copy.deepcopy(pcd)
    pcd_copy.rotate(R, center=(0, 0, 0))
    pcd_copy.translate(trans)
    return pcd_copy


def refine_icp(source, target, o3d=None, log=None):
    """Point-to-point ICP of source onto target (5 cm, identity start, up to 2000 iterations); source is moved by the
    result and returned."""
    o3d = o3d or _default_o3d()
    if log:
        log("   Running ICP...")
    reg = o3d.pipelines.registration.registration_icp(
        source, target, ICP_MAX_CORRESPONDENCE_DISTANCE, np.eye(4),
        o3d.pipelines.registration.TransformationEstimationPointToPoint(),
        o3d.pipelines.registration.ICPConvergenceCriteria(max_iteration=ICP_MAX_ITERATION))
    source.transform(reg.transformation)
    return source


def calculate_metrics(source_pcd, target_gt, name="", log=None):
    """(accuracy, completeness) in cm: the mean nearest-neighbour distance map -> ground truth and back."""
    dists_map_to_gt = source_pcd.compute_point_cloud_distance(target_gt)
    accuracy = np.mean(dists_map_to_gt) * 100
    dists_gt_to_map = target_gt.compute_point_cloud_distance(source_pcd)
    completeness = np.mean(dists_gt_to_map) * 100
    if log:
        log(f"Evaluating {name}: accuracy {accuracy:.2f} cm, completeness {completeness:.2f} cm")
    return accuracy, completeness
