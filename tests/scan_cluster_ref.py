"""numpy restatement of the object trigger's three stages (DESIGN.md §4 "scan clustering"), written from the reference
lines with every cast explicit: the checker of test_scan_cluster_api.py and test_gpu_scan_cluster.py.

* ``cluster_scan``          lidar_cluster_publisher.cpp:151-291 (one scan)
* ``object_map_filter``     object_filter.cpp:51-155 (one scan)
* ``cluster_observations``  3_multi_object_goal_selector.cpp:172-215 (one cloud)

float32 wherever the node holds a float, float64 where it holds a double.  cosf / sinf are libm's (the functions the
node links; numpy's float32 cos / sin are another implementation), hypotf is the float rounding of the double
sqrt(x^2 + y^2).  Linearity is the float64 definition of DESIGN.md §4, not Eigen's float evaluation.  A single kept
cluster whose ends meet across the seam is kept once (the node's self-insert is undefined behaviour).
"""
import ctypes
import ctypes.util
import math
from dataclasses import dataclass

import numpy as np

F = np.float32
NONE, WALL, OBJECT, UNKNOWN = 0, 1, 2, 3

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]


@dataclass
class ClusterParams:  # lidar_cluster_publisher.cpp:73-102, the node's defaults
    gap_threshold: float = 0.2
    min_cluster_points: int = 1
    max_range_ratio: float = 1.0
    obj_len_max: float = 1.0
    wal_len_min: float = 2.0
    wal_lin_max: float = 0.001
    obj_nmp_min: int = 1
    wal_nmp_min: int = 20


@dataclass
class ObservationParams:  # 3_multi_object_goal_selector.cpp:41-45
    cluster_distance_threshold: float = 0.4
    min_cluster_points: int = 10
    wall_thickness_threshold: float = 0.2
    lock_margin: float = 0.5


def beam_dirs(n_beams, angle_min, angle_increment):
    """(cos, sin) float32 [n] of angle = angle_min + i * angle_increment, all float (:165-167)"""
    a = F(angle_min) + np.arange(n_beams, dtype=np.float32) * F(angle_increment)
    c = np.array([_libm.cosf(float(v)) for v in a], np.float32)
    s = np.array([_libm.sinf(float(v)) for v in a], np.float32)
    return c, s


def hypot_f(dx, dy):
    dx, dy = np.float64(dx), np.float64(dy)
    return F(np.sqrt(dx * dx + dy * dy))


def _size_t(v):  # static_cast<size_t>(int)
    return int(v) % (1 << 64)


def pose_rows(pose):
    """rows 0 / 1 of tf2's Matrix3x3::setRotation(q) and the translation; None = identity"""
    if pose is None:
        return 1.0, 0.0, 0.0, 1.0, 0.0, 0.0
    tx, ty, _, x, y, z, w = (float(v) for v in pose)
    d = ((x * x + y * y) + z * z) + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wz, xx, xy, yy, zz = w * zs, x * xs, x * ys, y * ys, z * zs
    return 1.0 - (yy + zz), xy - wz, xy + wz, 1.0 - (xx + zz), tx, ty


def apply_pose(rows, x, y):
    m00, m01, m10, m11, tx, ty = rows
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return ((x * m00 + y * m01) + tx).astype(F), ((x * m10 + y * m11) + ty).astype(F)


def length_of(xs, ys):
    """computeClusterLength (:114-127), float"""
    mnx, mxx = min(F(1e6), xs.min()), max(F(-1e6), xs.max())
    mny, mxy = min(F(1e6), ys.min()), max(F(-1e6), ys.max())
    dx, dy = F(mxx - mnx), F(mxy - mny)
    return F(np.sqrt(F(F(dx * dx) + F(dy * dy))))


def linearity_of(xs, ys):
    """the float64 definition: mean of the widened points, centred sums / (n - 1), closed-form eigenvalues"""
    n = xs.size
    if n < 3:
        return 0.0
    X, Y = xs.astype(np.float64), ys.astype(np.float64)
    dx, dy = X - X.sum() / n, Y - Y.sum() / n
    a, b, c = (dx * dx).sum() / (n - 1), (dx * dy).sum() / (n - 1), (dy * dy).sum() / (n - 1)
    half, hd = (a + c) / 2.0, (a - c) / 2.0
    root = math.sqrt(hd * hd + b * b)
    l0, l1 = half - root, half + root
    if l0 + l1 < 1e-6:
        return 0.0
    return float(l0 / (l1 + 1e-6))


def classify(length, linearity, n, p):
    """:245-256; the thresholds are float members, the counts compare as size_t"""
    if linearity < float(F(p.wal_lin_max)) and length > F(p.wal_len_min) and n > _size_t(p.wal_nmp_min):
        return WALL
    if length < F(p.obj_len_max) and n > _size_t(p.obj_nmp_min):
        return OBJECT
    return UNKNOWN


class ScanClusters:
    pass


def cluster_scan(ranges, dirs, range_max, pose=None, p=ClusterParams()):
    r = np.asarray(ranges, np.float32)
    c, s = dirs
    n = r.size
    use = F(F(range_max) * F(p.max_range_ratio))  # :153
    with np.errstate(invalid="ignore"):
        valid = ~(np.isnan(r) | np.isinf(r)) & ~(r > use)
        x, y = (r * c).astype(F), (r * s).astype(F)
    gap = F(p.gap_threshold)
    clusters, cur = [], []
    for i in np.nonzero(valid)[0]:
        if cur:
            j = cur[-1]
            if hypot_f(x[i] - x[j], y[i] - y[j]) > gap:  # :172-173
                if len(cur) >= _size_t(p.min_cluster_points):
                    clusters.append(cur)
                cur = []
        cur.append(int(i))
    if cur and len(cur) >= _size_t(p.min_cluster_points):
        clusters.append(cur)
    out = ScanClusters()
    out.merged = out.ring = False
    if clusters:  # :186-199
        a, b = clusters[-1][-1], clusters[0][0]
        if hypot_f(x[a] - x[b], y[a] - y[b]) < gap:
            if len(clusters) >= 2:
                clusters[-1] = clusters[-1] + clusters[0]
                clusters.pop(0)
                out.merged = True
            else:
                out.ring = True  # kept once: the divergence of DESIGN.md §4
    rows = pose_rows(pose)
    out.n_clusters = len(clusters)
    out.beam_cluster = np.full(n, -1, np.int32)
    out.beam_class = np.zeros(n, np.uint8)
    out.beam_xy = np.full((n, 2), np.nan, np.float32)
    bx, by = apply_pose(rows, x[valid], y[valid])
    out.beam_xy[valid, 0], out.beam_xy[valid, 1] = bx, by
    out.first_beam = np.zeros(len(clusters), np.int32)
    out.n_points = np.zeros(len(clusters), np.int32)
    out.length = np.zeros(len(clusters), np.float32)
    out.linearity = np.zeros(len(clusters), np.float64)
    out.cls = np.zeros(len(clusters), np.int32)
    clouds = {WALL: [], OBJECT: [], UNKNOWN: []}
    for k, idx in enumerate(clusters):
        idx = np.asarray(idx)
        xs, ys = x[idx], y[idx]
        out.first_beam[k], out.n_points[k] = idx[0], idx.size
        out.length[k] = length_of(xs, ys)
        out.linearity[k] = linearity_of(xs, ys)
        out.cls[k] = classify(out.length[k], out.linearity[k], idx.size, p)
        out.beam_cluster[idx] = k
        out.beam_class[idx] = out.cls[k]
        clouds[int(out.cls[k])].append(np.stack([out.beam_xy[idx, 0], out.beam_xy[idx, 1],
                                                 np.zeros(idx.size, np.float32)], axis=1))
    out.clouds = {k: (np.concatenate(v) if v else np.zeros((0, 3), np.float32)) for k, v in clouds.items()}
    return out


def object_map_filter(obj_xyz, virtual_ranges, dirs, range_max, pose=None, proximity_threshold=0.5):
    """(keep mask, kept points) of one scan's object points against the walls of its virtual scan"""
    obj = np.asarray(obj_xyz, np.float32).reshape(-1, 3)
    r = np.asarray(virtual_ranges, np.float32)
    c, s = dirs
    with np.errstate(invalid="ignore"):
        ok = ~(np.isinf(r) | np.isnan(r) | (r > F(range_max)))  # :66
    lx, ly = (r[ok] * c[ok]).astype(np.float64), (r[ok] * s[ok]).astype(np.float64)
    if pose is None:
        tx, ty, cy, sy = 0.0, 0.0, 1.0, 0.0
    else:
        tx, ty, _, qx, qy, qz, qw = (float(v) for v in pose)
        yaw = math.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))  # :166
        cy, sy = math.cos(yaw), math.sin(yaw)
    wx = tx + (lx * cy - ly * sy)  # :168-169
    wy = ty + (lx * sy + ly * cy)
    keep = np.zeros(obj.shape[0], bool)
    if wx.size:  # :93
        p2 = float(proximity_threshold) * float(proximity_threshold)
        for i in range(obj.shape[0]):
            dx = (np.float64(obj[i, 0]) - wx).astype(F)  # :121-122
            dy = (np.float64(obj[i, 1]) - wy).astype(F)
            d2 = (dx * dx + dy * dy).astype(np.float64)  # float sum, compared in double (:124)
            keep[i] = not bool((d2 < p2).any())
    return keep, obj[keep]


def cluster_observations(points, pose=None, p=ObservationParams()):
    """rows (cx, cy, width, height, lock_radius) float32 [k][5] of one cloud, and how many clusters each rule
    rejected: (below min_cluster_points, thinner than wall_thickness_threshold)"""
    pts = np.asarray(points, np.float32)
    x, y = pts[:, 0], pts[:, 1]
    n = x.size
    rows, small, thin = [], 0, 0
    if n == 0:  # :176
        return np.zeros((0, 5), np.float32), small, thin
    clusters, cur = [], [0]
    for i in range(1, n):
        dx, dy = F(x[i] - x[i - 1]), F(y[i] - y[i - 1])
        if float(np.sqrt(F(F(dx * dx) + F(dy * dy)))) > float(p.cluster_distance_threshold):  # :184
            clusters.append(cur)
            cur = []
        cur.append(i)
    clusters.append(cur)
    M = pose_rows(pose)
    for idx in clusters:
        if not len(idx) >= _size_t(p.min_cluster_points):  # :185, :190
            small += 1
            continue
        xs, ys = x[idx], y[idx]
        mnx, mxx = min(F(1e6), xs.min()), max(F(-1e6), xs.max())
        mny, mxy = min(F(1e6), ys.min()), max(F(-1e6), ys.max())
        w, h = F(mxx - mnx), F(mxy - mny)
        if float(min(w, h)) < float(p.wall_thickness_threshold):  # :200
            thin += 1
            continue
        lcx, lcy = F(F(mnx + mxx) / F(2.0)), F(F(mny + mxy) / F(2.0))
        cx, cy = apply_pose(M, lcx, lcy)
        diagonal = F(np.sqrt(F(F(w * w) + F(h * h))))  # :135
        lock = F(float(F(diagonal / F(2.0))) + float(p.lock_margin))  # :136
        rows.append([F(cx), F(cy), w, h, lock])
    return np.asarray(rows, np.float32).reshape(-1, 5), small, thin
