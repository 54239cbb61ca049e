"""The object trigger's entry points (ot_scan_cluster, ot_object_map_filter, ot_cluster_observations) validate their
arguments before any device work, and known-answer cases for the numpy restatement the GPU tests check against
(scan_cluster_ref.py).  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import scan_cluster_ref as R

F = np.float32


# ------------------------------------------------------------------------------------------------ argument validation
def _cluster_args(pkg, n_scans, n_beams, buffers, params=True, min_cluster_points=1):
    cd = pkg.change_detection
    prm = cd._ClusterParams(0.2, min_cluster_points, 1.0, 1.0, 2.0, 0.001, 1, 20)
    off = (C.c_int64 * (3 * (max(n_scans, 0) + 1)))()
    b = C.c_void_p(buffers)
    return [b, n_scans, n_beams, 0.0, 0.1, 10.0, None, C.byref(prm) if params else None, b, b, b, b, b, b, b, b, off,
            None]


@pytest.mark.parametrize("case", ["null_buffers", "zero_beams", "negative_beams", "null_params", "too_many_beams",
                                  "min_points_zero"])
def test_scan_cluster_rejects_bad_arguments(pkg, case):
    lib = pkg.native_library()
    fake = 4096  # never dereferenced: every case is refused before any device work
    args = {"null_buffers": _cluster_args(pkg, 1, 16, None),
            "zero_beams": _cluster_args(pkg, 1, 0, fake),
            "negative_beams": _cluster_args(pkg, 1, -3, fake),
            "null_params": _cluster_args(pkg, 1, 16, fake, params=False),
            "too_many_beams": _cluster_args(pkg, 1, 4097, fake),
            "min_points_zero": _cluster_args(pkg, 1, 16, fake, min_cluster_points=0)}[case]
    assert lib.ot_scan_cluster(*args) == pkg._lib.OT_ERR_INVALID_ARGUMENT
    msg = lib.ot_last_error()
    assert b"LidarClusterer" in msg
    if case == "too_many_beams":
        assert b"4097" in msg and b"4096" in msg


def test_scan_cluster_zero_scans_is_legal(pkg):
    lib = pkg.native_library()
    args = _cluster_args(pkg, 0, 16, None)
    args[16][0] = args[16][1] = args[16][2] = 7
    assert lib.ot_scan_cluster(*args) == pkg._lib.OT_OK
    assert list(args[16]) == [0, 0, 0]


@pytest.mark.parametrize("case", ["null_buffers", "zero_beams", "null_offsets", "decreasing_offsets"])
def test_object_map_filter_rejects_bad_arguments(pkg, case):
    lib = pkg.native_library()
    off = (C.c_int64 * 2)(0, 5)
    bad = (C.c_int64 * 2)(0, -1)
    out = (C.c_int64 * 2)()
    fake = C.c_void_p(4096)
    args = {"null_buffers": [None, off, 1, None, 16, 0.0, 0.1, 10.0, None, 0.5, None, None, out, None],
            "zero_beams": [fake, off, 1, fake, 0, 0.0, 0.1, 10.0, None, 0.5, fake, fake, out, None],
            "null_offsets": [fake, None, 1, fake, 16, 0.0, 0.1, 10.0, None, 0.5, fake, fake, out, None],
            "decreasing_offsets": [fake, bad, 1, fake, 16, 0.0, 0.1, 10.0, None, 0.5, fake, fake, out, None]}[case]
    assert lib.ot_object_map_filter(*args) == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert b"ObjectMapFilter" in lib.ot_last_error()


def test_object_map_filter_empty_object_list_is_legal(pkg):
    lib = pkg.native_library()
    off = (C.c_int64 * 3)(0, 0, 0)
    out = (C.c_int64 * 3)(9, 9, 9)
    assert lib.ot_object_map_filter(None, off, 2, None, 16, 0.0, 0.1, 10.0, None, 0.5, None, None, out,
                                    None) == pkg._lib.OT_OK
    assert list(out) == [0, 0, 0]


@pytest.mark.parametrize("case", ["null_buffers", "null_params", "bad_stride", "too_many_points"])
def test_cluster_observations_rejects_bad_arguments(pkg, case):
    lib = pkg.native_library()
    prm = pkg.change_detection._ObservationParams(0.4, 0.2, 0.5, 10)
    off = (C.c_int64 * 2)(0, 5)
    big = (C.c_int64 * 2)(0, 4097)
    n_obs = (C.c_int32 * 1)()
    fake = C.c_void_p(4096)
    args = {"null_buffers": [None, 3, off, 1, None, C.byref(prm), None, n_obs, None],
            "null_params": [fake, 3, off, 1, None, None, fake, n_obs, None],
            "bad_stride": [fake, 1, off, 1, None, C.byref(prm), fake, n_obs, None],
            "too_many_points": [fake, 3, big, 1, None, C.byref(prm), fake, n_obs, None]}[case]
    assert lib.ot_cluster_observations(*args) == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert b"cluster_observations" in lib.ot_last_error()


def test_parameter_structs_match_the_header(pkg):
    cd = pkg.change_detection
    assert C.sizeof(cd._ClusterParams) == 32 and cd.CLUSTER_ROW.itemsize == 24
    assert C.sizeof(cd._ObservationParams) == 32
    d = cd.LidarClusterer()._params  # the node's defaults (lidar_cluster_publisher.cpp:73-86)
    assert (d.gap_threshold, d.min_cluster_points, d.max_range_ratio, d.obj_len_max, d.wal_len_min, d.obj_nmp_min,
            d.wal_nmp_min) == (F(0.2), 1, 1.0, 1.0, 2.0, 1, 20)
    assert d.wal_lin_max == F(0.001)


# ------------------------------------------------------------------------------------------------ the restatement
def _dirs(n):
    return R.beam_dirs(n, -np.pi, 2 * np.pi / n)


def test_all_invalid_scan():
    r = np.array([np.nan, np.inf, -np.inf, 20.0] * 4, np.float32)
    c = R.cluster_scan(r, _dirs(16), 12.0)
    assert c.n_clusters == 0 and (c.beam_cluster == -1).all() and (c.beam_class == 0).all()
    assert np.isnan(c.beam_xy).all()
    assert all(v.shape == (0, 3) for v in c.clouds.values())


def test_constant_ring_is_one_cluster_kept_once():
    n = 64
    c = R.cluster_scan(np.full(n, 1.0, np.float32), _dirs(n), 12.0)  # neighbours 0.098 m apart, seam included
    assert c.ring and not c.merged and c.n_clusters == 1
    assert c.n_points[0] == n and c.first_beam[0] == 0
    assert c.cls[0] == R.UNKNOWN  # a circle: length 2.83 m, linearity ~1
    assert c.clouds[R.UNKNOWN].shape == (n, 3) and (c.beam_cluster == 0).all()
    assert abs(c.linearity[0] - 1.0) < 1e-3 and abs(float(c.length[0]) - 2 * np.sqrt(2)) < 1e-3


def test_seam_merge_puts_the_merged_cluster_last():
    n = 64
    r = np.full(n, np.inf, np.float32)
    r[0:4] = 1.0    # arc A starts at beam 0 ...
    r[20:30] = 1.0  # arc B
    r[60:64] = 1.0  # ... and continues arc C across the seam
    c = R.cluster_scan(r, _dirs(n), 12.0)
    assert c.merged and c.n_clusters == 2
    assert c.first_beam.tolist() == [20, 60] and c.n_points.tolist() == [10, 8]
    assert (c.beam_cluster[0:4] == 1).all() and (c.beam_cluster[60:64] == 1).all() and \
        (c.beam_cluster[20:30] == 0).all()
    # all three arcs are short OBJECT clusters: the cloud starts after the seam cluster (B), then C's points, then A's
    assert c.cls.tolist() == [R.OBJECT, R.OBJECT]
    order = list(range(20, 30)) + list(range(60, 64)) + list(range(0, 4))
    assert np.array_equal(c.clouds[R.OBJECT][:, :2], c.beam_xy[order])
    assert (c.clouds[R.OBJECT][:, 2] == 0).all()


def test_min_cluster_points_drops_specks_and_keeps_their_breaks():
    n = 64
    r = np.full(n, np.inf, np.float32)
    r[0] = 1.0       # 1-beam speck at the scan start
    r[3:5] = 2.0     # 2-beam speck
    r[10:20] = 1.0   # the first kept cluster
    r[40:50] = 1.5
    r[62:64] = 1.0   # 2-beam speck next to beam 0 across the seam: dropped, so no merge through it
    p = R.ClusterParams(min_cluster_points=3)
    c = R.cluster_scan(r, _dirs(n), 12.0, p=p)
    assert c.n_clusters == 2 and not c.merged and not c.ring
    assert c.first_beam.tolist() == [10, 40]
    assert (c.beam_cluster[[0, 3, 4, 62, 63]] == -1).all() and (c.beam_class[[0, 3, 4, 62, 63]] == 0).all()
    assert not np.isnan(c.beam_xy[[0, 3, 4, 62, 63]]).any()  # valid beams keep their map-frame point


def test_straight_segment_is_a_wall_and_a_pair_is_an_object():
    n = 720
    cs, sn = _dirs(n)
    r = np.full(n, np.inf, np.float32)
    with np.errstate(divide="ignore"):
        line = (2.0 / cs.astype(np.float64)).astype(np.float32)  # the wall x = 2
    sel = np.arange(n)[(cs > 0) & (np.abs(2.0 * sn / np.where(cs > 0, cs, 1.0)) < 1.6)]
    r[sel] = line[sel]
    r[100:102] = 1.0  # a 2-beam cluster
    c = R.cluster_scan(r, (cs, sn), 12.0)
    k = int(c.beam_cluster[sel[0]])
    assert c.n_points[k] == sel.size > 20 and c.length[k] > 2.0
    assert c.linearity[k] < 1e-6 and c.cls[k] == R.WALL
    j = int(c.beam_cluster[100])
    assert c.n_points[j] == 2 and c.linearity[j] == 0.0 and c.cls[j] == R.OBJECT


def test_object_filter_and_observations_restatement():
    d = _dirs(64)
    virt = np.full(64, np.inf, np.float32)
    virt[32] = 2.0  # one wall point at (2, 0) (beam 32 looks along +x)
    obj = np.array([[2.3, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)
    keep, kept = R.object_map_filter(obj, virt, d, 12.0)
    assert keep.tolist() == [False, True] and kept.shape == (1, 3)
    keep, _ = R.object_map_filter(obj, np.full(64, np.inf, np.float32), d, 12.0)
    assert not keep.any()  # no wall points: the node returns early
    # a 12-point 0.3 x 0.3 blob, a thin 12-point line, a 3-point blob
    t = np.linspace(0, 1, 12)
    blob = np.stack([0.3 * t, 0.3 * np.sin(7 * t) ** 2], axis=1)
    thin = np.stack([5 + 0.3 * t, np.zeros(12)], axis=1)
    short = np.array([[9.0, 9.0], [9.1, 9.3], [9.3, 9.1]])
    rows, small, thinned = R.cluster_observations(np.concatenate([blob, thin, short]).astype(np.float32))
    assert rows.shape == (1, 5) and small == 1 and thinned == 1
    w, h = rows[0, 2], rows[0, 3]
    assert rows[0, 4] == F(float(F(np.sqrt(F(w * w + h * h)) / F(2.0))) + 0.5)
