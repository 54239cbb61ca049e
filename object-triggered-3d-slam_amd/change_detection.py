"""Change detection against a saved map — SURVEY.md §8(f) rank 2, BASELINE configs[4] ("diff vs saved map").

Host-side mirrors of the reference's change-detection code, backed by the HIP kernels of libotslam_hip.so:

* ``smart_paste(base_img, overlay_img, x, y, w, h)`` — fusion/2d_selective_merge.py:58-69 (same signature; the
  base grid is updated in place and returned, as the reference does).
* ``ChangeDetector`` — ros2_ws/src/lidar_detection/src/diff_node.cpp (ChangeDetectorNode): the node's parameters
  (distance_threshold, time_threshold, grid_resolution, decay_rate) and its per-scan callback, with the beam
  comparison batched over many scans on the GPU and the time-decayed evidence grid kept in native host code.
* ``voxel_key_diff(new, old, voxel_size, origin)`` — added / removed lattice cells of an object cloud versus the
  saved map's cloud (the 3-D half of configs[4]'s diff).
* ``virtual_scan(grid, resolution, origin, template, poses)`` — ros2_ws/src/lidar_detection/src/virtual_scan_node.cpp
  (VirtualScanNode): the scan the saved map would return at each robot pose (the diff node's /virtual_scan input),
  ray-marched per beam on the GPU; ``occupancy_from_pgm`` / ``tf2_get_yaw`` prepare its inputs.

* ``LidarClusterer`` / ``ObjectMapFilter`` / ``cluster_observations`` — the object trigger between the scans and
  the ScanObject goal: lidar_cluster_publisher.cpp (gap clusters of a scan, WALL / OBJECT / UNKNOWN),
  object_filter.cpp (object points near a wall of the virtual scan are dropped) and the clustering front half of
  3_multi_object_goal_selector.cpp (one observation per remaining cluster), each batched over scans.

Every compute call goes through the C ABI; there is no CPU implementation in this module.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _device as D
from . import _lib as L

UNKNOWN_PIXEL = 205  # 2d_selective_merge.py:63
PASTE_THRESHOLD = 5  # 2d_selective_merge.py:64


def smart_paste(base_img, overlay_img, x, y, w, h, unknown=UNKNOWN_PIXEL, threshold=PASTE_THRESHOLD):
    """2d_selective_merge.py:58-69: cells of ``overlay_img`` inside the rectangle that carry data (outside
    unknown ± threshold) overwrite ``base_img``.  Updates ``base_img`` (uint8 numpy array) in place and returns
    it; a rectangle reaching outside the image leaves it unchanged."""
    n_changed = _paste(base_img, overlay_img, x, y, w, h, unknown, threshold)
    del n_changed
    return base_img


def merge_maps(old_map, new_map, unknown=UNKNOWN_PIXEL, threshold=PASTE_THRESHOLD):
    """Whole-map smart_paste of a new occupancy grid onto the saved one.  Returns (merged copy, changed cells)."""
    out = np.array(old_map, dtype=np.uint8, copy=True)
    h, w = out.shape
    n = _paste(out, new_map, 0, 0, w, h, unknown, threshold)
    return out, n


def _paste(base_img, overlay_img, x, y, w, h, unknown, threshold):
    base = np.asarray(base_img)
    if base.dtype != np.uint8 or base.ndim != 2:
        raise RuntimeError("[smart_paste] base_img must be a 2-D uint8 grid")
    over = np.ascontiguousarray(overlay_img, dtype=np.uint8)
    if over.shape != base.shape:
        raise RuntimeError("[smart_paste] overlay_img must have the base grid's shape")
    hh, ww = base.shape
    if x < 0 or y < 0 or x + w > ww or y + h > hh or w <= 0 or h <= 0:
        return 0
    db = D.to_device(np.ascontiguousarray(base))
    do = D.to_device(over)
    n = C.c_int64(0)
    L.call("ot_grid_smart_paste", D.ptr(db), D.ptr(do), hh, ww, int(x), int(y), int(w), int(h), int(unknown),
           int(threshold), C.byref(n), D.stream_ptr())
    base[...] = D.to_host(db)
    return n.value


def voxel_key_diff(new_cloud, old_cloud, voxel_size, origin):
    """Lattice cells floor((p - origin) / voxel_size) occupied by ``new_cloud`` but not ``old_cloud`` (added) and
    the converse (removed); int32 [k][3] each, sorted lexicographically.  Clouds: PointCloud or (n, 3) arrays."""
    a = _xyz_dev(new_cloud)
    b = _xyz_dev(old_cloud)
    n, m = int(a.shape[0]), int(b.shape[0])
    added = D.empty((max(n, 1), 3), "int32")
    removed = D.empty((max(m, 1), 3), "int32")
    na, nr = C.c_int64(0), C.c_int64(0)
    o = (C.c_double * 3)(*[float(v) for v in origin])
    L.call("ot_voxel_key_diff", D.ptr(a) if n else None, n, D.ptr(b) if m else None, m, float(voxel_size), o,
           D.ptr(added), C.byref(na), D.ptr(removed), C.byref(nr), D.stream_ptr())
    return D.to_host(added[:na.value]), D.to_host(removed[:nr.value])


def voxel_key_diff_multi(new_clouds, old_clouds, voxel_size, origin):
    """voxel_key_diff for many objects in one pass (object j of new_clouds vs object j of old_clouds).  Returns
    (added, removed) as int32 [k][4] = (object, x, y, z), sorted by object then cell."""
    if len(new_clouds) != len(old_clouds):
        raise RuntimeError("[voxel_key_diff] new and old object lists differ in length")
    import torch

    def cat(clouds):
        parts = [_xyz_dev(c) for c in clouds]
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([int(p.shape[0]) for p in parts])
        xyz = torch.cat(parts, 0).contiguous() if parts else D.empty((0, 3), "float64")
        return xyz, off

    a, oa = cat(new_clouds)
    b, ob = cat(old_clouds)
    added = D.empty((max(int(oa[-1]), 1), 4), "int32")
    removed = D.empty((max(int(ob[-1]), 1), 4), "int32")
    na, nr = C.c_int64(0), C.c_int64(0)
    o = (C.c_double * 3)(*[float(v) for v in origin])
    L.call("ot_voxel_key_diff_multi", D.ptr(a) if oa[-1] else None, oa.ctypes.data_as(C.c_void_p),
           D.ptr(b) if ob[-1] else None, ob.ctypes.data_as(C.c_void_p), len(new_clouds), float(voxel_size), o,
           D.ptr(added), C.byref(na), D.ptr(removed), C.byref(nr), D.stream_ptr())
    return D.to_host(added[:na.value]), D.to_host(removed[:nr.value])


def _xyz_dev(c):
    if hasattr(c, "_xyz"):
        return c._xyz.dev()
    a = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1, 3))
    return D.to_device(a)


@dataclass
class LaserScan:
    """The sensor_msgs/LaserScan fields the change detector reads."""

    ranges: np.ndarray
    angle_min: float
    angle_increment: float
    range_max: float = float("inf")


class ChangeDetector:
    """ChangeDetectorNode (diff_node.cpp): compares each real scan with the virtual scan rendered from the saved
    map.  ``scan_callback`` handles one scan pair; ``process`` a batch of pairs (one GPU launch for all beams, then
    the evidence-grid updates in scan order).  Outputs are the node's two published clouds — added (new) and
    removed (gone) cells above time_threshold — as float32 (k, 3) arrays sorted by cell."""

    SEARCH_WINDOW = 20  # diff_node.cpp:113, :143

    def __init__(self, distance_threshold=0.5, time_threshold=2.0, grid_resolution=0.1, decay_rate=0.5):
        self.distance_threshold = float(distance_threshold)
        self.time_threshold = float(time_threshold)
        self.grid_resolution = float(grid_resolution)
        self.decay_rate = float(decay_rate)
        self._grids = []
        for _ in range(2):
            g = C.c_void_p()
            L.call("ot_change_grid_create", self.time_threshold, self.decay_rate, self.grid_resolution, C.byref(g))
            self._grids.append(g)

    def __del__(self):
        for g in getattr(self, "_grids", []):
            try:
                L.call("ot_change_grid_destroy", g)
            except Exception:
                pass

    def scan_callback(self, real_scan: LaserScan, virtual_scan: LaserScan, pose, dt):
        """One scan pair (pose = map<-sensor as (tx, ty, tz, qx, qy, qz, qw)); returns (added, removed)."""
        if len(real_scan.ranges) != len(virtual_scan.ranges):  # diff_node.cpp:87
            return self.published()
        return self.process(np.asarray(real_scan.ranges, np.float32)[None], np.asarray(virtual_scan.ranges,
                            np.float32)[None], real_scan, virtual_scan, np.asarray(pose, np.float64)[None], [dt])

    def process(self, real_ranges, virtual_ranges, real_meta: LaserScan, virtual_meta: LaserScan, poses, dts):
        """Batch of B scan pairs: ranges float32 [B][N], poses [B][7], dts [B] (seconds since the previous scan)."""
        flags_new, flags_gone, keys_new, keys_gone = self.flag_beams(real_ranges, virtual_ranges, real_meta,
                                                                     virtual_meta, poses)
        for b, dt in enumerate(dts):
            for g, k, f in ((self._grids[0], keys_new[b], flags_new[b]), (self._grids[1], keys_gone[b], flags_gone[b])):
                k = np.ascontiguousarray(k, np.int32)
                f = np.ascontiguousarray(f, np.uint8)
                L.call("ot_change_grid_update", g, k.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                       f.shape[0], float(dt))
        return self.published()

    def flag_beams(self, real_ranges, virtual_ranges, real_meta: LaserScan, virtual_meta: LaserScan, poses):
        """GPU part: per-beam new / gone flags and map-grid cells for B scans (diff_node.cpp:103-160)."""
        R = _as_dev(real_ranges, np.float32)
        V = _as_dev(virtual_ranges, np.float32)
        if R.shape != V.shape or R.dim() != 2:
            raise RuntimeError("[ChangeDetector] real and virtual ranges must both be [n_scans][n_beams]")
        B, N = int(R.shape[0]), int(R.shape[1])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(B, 7))
        fn, fg = D.empty((B, N), "uint8"), D.empty((B, N), "uint8")
        kn, kg = D.empty((B, N, 2), "int32"), D.empty((B, N, 2), "int32")
        L.call("ot_scan_diff", D.ptr(R), D.ptr(V), B, N, float(real_meta.angle_min), float(real_meta.angle_increment),
               float(real_meta.range_max), float(virtual_meta.angle_min), float(virtual_meta.angle_increment),
               self.distance_threshold, self.SEARCH_WINDOW, P.ctypes.data_as(C.c_void_p), self.grid_resolution,
               D.ptr(fn), D.ptr(fg), D.ptr(kn), D.ptr(kg), D.stream_ptr())
        return D.to_host(fn), D.to_host(fg), D.to_host(kn), D.to_host(kg)

    def published(self):
        """(added, removed): cells above time_threshold as float32 (x*res + res/2, y*res + res/2, 0)."""
        out = []
        for g in self._grids:
            n = C.c_int64(0)
            L.call("ot_change_grid_publish", g, None, 0, C.byref(n))
            xyz = np.zeros((n.value, 3), np.float32)
            if n.value:
                L.call("ot_change_grid_publish", g, xyz.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
            out.append(xyz)
        return out[0], out[1]


def tf2_get_yaw(qx, qy, qz, qw):
    """tf2::getYaw(quaternion) (tf2/utils.h: Matrix3x3(q).getEulerYPR): yaw of the rotation matrix of q."""
    d = qx * qx + qy * qy + qz * qz + qw * qw
    s = 2.0 / d
    xs, ys, zs = qx * s, qy * s, qz * s
    wz, xx, xy = qw * zs, qx * xs, qx * ys
    yy, zz = qy * ys, qz * zs
    m00, m10, m20 = 1.0 - (yy + zz), xy + wz, qx * zs - qw * ys
    if abs(m20) >= 1:  # gimbal lock: tf2 returns yaw 0
        return 0.0
    cp = np.cos(-np.arcsin(m20))
    return float(np.arctan2(m10 / cp, m00 / cp))


def occupancy_from_pgm(img, negate=0, occupied_thresh=0.65, free_thresh=0.196):
    """map_server's trinary PGM -> OccupancyGrid data (int8: 100 occupied, 0 free, -1 unknown)."""
    v = np.asarray(img, dtype=np.float64)
    p = v / 255.0 if negate else (255.0 - v) / 255.0
    out = np.full(v.shape, -1, np.int8)
    out[p > occupied_thresh] = 100
    out[p < free_thresh] = 0
    return out[::-1].copy()  # PGM row 0 is the top of the map; OccupancyGrid row 0 is the bottom (origin)


def virtual_scan(grid, resolution, origin, template: LaserScan, poses, n_beams=None):
    """virtual_scan_node.cpp:245-292 (VirtualScanNode, "copycat" mode): the LaserScan the saved map would produce
    at each robot pose, with the template scan's angles and range_max.  grid: OccupancyGrid int8 [h][w]
    (row 0 at origin); poses [B][3] = (x, y, yaw).  Returns float32 ranges [B][n_beams] (+inf = no hit)."""
    g = _as_dev(grid, np.int8)
    if g.dim() != 2:
        raise RuntimeError("[VirtualScan] grid must be [height][width]")
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 3))
    n = int(n_beams if n_beams is not None else len(template.ranges))
    out = D.empty((P.shape[0], n), "float32")
    L.call("ot_virtual_scan", D.ptr(g), int(g.shape[0]), int(g.shape[1]), float(resolution), float(origin[0]),
           float(origin[1]), P.shape[0], n, float(template.angle_min), float(template.angle_increment),
           float(template.range_max), P.ctypes.data_as(C.c_void_p), D.ptr(out), D.stream_ptr())
    return D.to_host(out)


def _as_dev(a, dtype):
    if D.is_tensor(a):
        return a.contiguous()
    return D.to_device(np.ascontiguousarray(np.asarray(a, dtype=dtype)))


# ------------------------------------------------------------------------------------------------ object trigger
SCAN_CLASS_NONE, SCAN_CLASS_WALL, SCAN_CLASS_OBJECT, SCAN_CLASS_UNKNOWN = 0, 1, 2, 3
CLUSTER_ROW = np.dtype([("first_beam", "<i4"), ("n_points", "<i4"), ("length", "<f4"), ("cls", "<i4"),
                        ("linearity", "<f8")])  # ot_scan_cluster_row


class _ClusterParams(C.Structure):  # ot_scan_cluster_params
    _fields_ = [("gap_threshold", C.c_float), ("min_cluster_points", C.c_int32), ("max_range_ratio", C.c_float),
                ("obj_len_max", C.c_float), ("wal_len_min", C.c_float), ("wal_lin_max", C.c_float),
                ("obj_nmp_min", C.c_int32), ("wal_nmp_min", C.c_int32)]


class _ObservationParams(C.Structure):  # ot_observation_params
    _fields_ = [("cluster_distance_threshold", C.c_double), ("wall_thickness_threshold", C.c_double),
                ("lock_margin", C.c_double), ("min_cluster_points", C.c_int32)]


def _poses7(poses, n):
    if poses is None:
        return None, None
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(n, 7))
    return P, P.ctypes.data_as(C.c_void_p)


@dataclass
class ScanClusters:
    """LidarClusterer.process's result for S scans of N beams.  Per beam (numpy): ``beam_cluster`` int32 [S][N] (index
    in the scan's cluster list, -1 = none), ``beam_class`` uint8 [S][N] (SCAN_CLASS_*), ``beam_xy`` float32 [S][N][2]
    (map frame; NaN for invalid beams).  ``clusters[s]``: the scan's cluster table (CLUSTER_ROW records).  The
    three published clouds stay on the device, concatenated over scans (``wall_xyz`` / ``object_xyz`` /
    ``unknown_xyz`` float32 [k][3]) with host row offsets int64 [S + 1] (``wall_offsets`` ...); ``wall_cloud(s)``,
    ``object_cloud(s)``, ``unknown_cloud(s)`` return one scan's cloud as numpy."""

    beam_cluster: np.ndarray
    beam_class: np.ndarray
    beam_xy: np.ndarray
    n_clusters: np.ndarray
    clusters: list
    wall_xyz: object
    object_xyz: object
    unknown_xyz: object
    wall_offsets: np.ndarray
    object_offsets: np.ndarray
    unknown_offsets: np.ndarray

    def wall_cloud(self, s):
        return D.to_host(self.wall_xyz[self.wall_offsets[s]:self.wall_offsets[s + 1]])

    def object_cloud(self, s):
        return D.to_host(self.object_xyz[self.object_offsets[s]:self.object_offsets[s + 1]])

    def unknown_cloud(self, s):
        return D.to_host(self.unknown_xyz[self.unknown_offsets[s]:self.unknown_offsets[s + 1]])


class LidarClusterer:
    """LidarClusterPublisher (lidar_cluster_publisher.cpp): the node's parameters with its defaults and its scan
    callback, batched over scans on the GPU (ot_scan_cluster).  Linearity is the float64 definition of DESIGN.md §4;
    a single cluster closing on itself across the seam is kept once."""

    def __init__(self, gap_threshold=0.2, min_cluster_points=1, max_range_ratio=1.0, obj_len_max=1.0,
                 wal_len_min=2.0, wal_lin_max=0.001, obj_nmp_min=1, wal_nmp_min=20):
        self._params = _ClusterParams(float(gap_threshold), int(min_cluster_points), float(max_range_ratio),
                                      float(obj_len_max), float(wal_len_min), float(wal_lin_max), int(obj_nmp_min),
                                      int(wal_nmp_min))

    def process(self, ranges, meta: LaserScan, poses=None) -> ScanClusters:
        """ranges float32 [S][N] (numpy or device tensor), meta: the scans' angle_min / angle_increment / range_max,
        poses [S][7] = (tx, ty, tz, qx, qy, qz, qw) map <- base_link (None = identity)."""
        R = _as_dev(ranges, np.float32)
        if R.dim() != 2:
            raise RuntimeError("[LidarClusterer] ranges must be [n_scans][n_beams]")
        S, N = int(R.shape[0]), int(R.shape[1])
        P, pp = _poses7(poses, S)
        bc, bk = D.empty((S, N), "int32"), D.empty((S, N), "uint8")
        bxy = D.empty((S, N, 2), "float32")
        nc = D.empty((S,), "int32")
        rows = D.empty((S, N * CLUSTER_ROW.itemsize), "uint8")
        clouds = [D.empty((max(S * N, 1), 3), "float32") for _ in range(3)]
        off = np.zeros((3, S + 1), np.int64)
        L.call("ot_scan_cluster", D.ptr(R), S, N, float(meta.angle_min), float(meta.angle_increment),
               float(meta.range_max), pp, C.byref(self._params), D.ptr(bc), D.ptr(bk), D.ptr(bxy), D.ptr(nc),
               D.ptr(rows), D.ptr(clouds[0]), D.ptr(clouds[1]), D.ptr(clouds[2]), off.ctypes.data_as(C.c_void_p),
               D.stream_ptr())
        n_clusters = D.to_host(nc)
        table = D.to_host(rows).view(CLUSTER_ROW).reshape(S, N) if S else np.zeros((0, N), CLUSTER_ROW)
        return ScanClusters(D.to_host(bc), D.to_host(bk), D.to_host(bxy), n_clusters,
                            [table[s, :n_clusters[s]].copy() for s in range(S)],
                            clouds[0][:off[0, S]], clouds[1][:off[1, S]], clouds[2][:off[2, S]], off[0], off[1], off[2])


class ObjectMapFilter:
    """ObjectMapFilter (object_filter.cpp), batched over scans (ot_object_map_filter): object points within
    proximity_threshold of a wall point of the scan's virtual scan are dropped."""

    def __init__(self, proximity_threshold=0.5):
        self.proximity_threshold = float(proximity_threshold)

    def process(self, object_xyz, offsets, virtual_ranges, virtual_meta: LaserScan, poses=None):
        """object_xyz float32 [n][3] concatenated over scans (numpy or device tensor) with row offsets [S + 1];
        virtual_ranges float32 [S][N]; poses [S][7] map <- scan frame (None = identity).  Returns (kept points as a
        device tensor [k][3], their offsets int64 [S + 1], keep mask uint8 [n] numpy)."""
        V = _as_dev(virtual_ranges, np.float32)
        if V.dim() != 2:
            raise RuntimeError("[ObjectMapFilter] virtual_ranges must be [n_scans][n_beams]")
        S, N = int(V.shape[0]), int(V.shape[1])
        off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(S + 1))
        O = _as_dev(object_xyz, np.float32).reshape(-1, 3)
        n = int(O.shape[0])
        if n != int(off[-1]):
            raise RuntimeError("[ObjectMapFilter] offsets do not cover object_xyz")
        P, pp = _poses7(poses, S)
        mask = D.empty((max(n, 1),), "uint8")
        out = D.empty((max(n, 1), 3), "float32")
        out_off = np.zeros(S + 1, np.int64)
        L.call("ot_object_map_filter", D.ptr(O) if n else None, off.ctypes.data_as(C.c_void_p), S, D.ptr(V), N,
               float(virtual_meta.angle_min), float(virtual_meta.angle_increment), float(virtual_meta.range_max), pp,
               self.proximity_threshold, D.ptr(mask), D.ptr(out), out_off.ctypes.data_as(C.c_void_p), D.stream_ptr())
        return out[:out_off[S]], out_off, D.to_host(mask[:n])


def cluster_observations(points, offsets, poses=None, cluster_distance_threshold=0.4, min_cluster_points=10,
                         wall_thickness_threshold=0.2, lock_margin=0.5):
    """3_multi_object_goal_selector.cpp:172-215 (ot_cluster_observations): float32 points [n][2 or 3] (numpy or device
    tensor) of several clouds in message order with row offsets [n_clouds + 1]; poses [n_clouds][7] global <- cloud
    frame (None = identity).  Returns one float32 [k][5] array per cloud: (cx, cy, width, height, lock_radius) of its
    clusters, in cluster order.  The candidate / stable tracker that consumes them is host state outside this
    package."""
    X = _as_dev(points, np.float32)
    if X.dim() != 2 or int(X.shape[1]) not in (2, 3):
        raise RuntimeError("[cluster_observations] points must be [n][2] or [n][3]")
    off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    J, n = off.size - 1, int(X.shape[0])
    if J < 0 or n != int(off[-1]):
        raise RuntimeError("[cluster_observations] offsets do not cover points")
    P, pp = _poses7(poses, J)
    prm = _ObservationParams(float(cluster_distance_threshold), float(wall_thickness_threshold), float(lock_margin),
                             int(min_cluster_points))
    rows = D.empty((max(n, 1), 5), "float32")
    n_obs = np.zeros(max(J, 1), np.int32)
    L.call("ot_cluster_observations", D.ptr(X) if n else None, int(X.shape[1]), off.ctypes.data_as(C.c_void_p), J, pp,
           C.byref(prm), D.ptr(rows), n_obs.ctypes.data_as(C.c_void_p), D.stream_ptr())
    return [D.to_host(rows[off[j]:off[j] + n_obs[j]]) for j in range(J)]
