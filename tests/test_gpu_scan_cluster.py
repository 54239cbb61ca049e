"""GPU parity of the object trigger (LidarClusterer, ObjectMapFilter, cluster_observations) against the numpy
restatement in scan_cluster_ref.py ("scan clustering").

Everything is bit-exact except the linearity, whose summation order inside a cluster is free: sums of <= 4096 doubles
differ between orders by at most about N 2^-53 ~ 5e-13 relative, <~ 1e-12 on the eigenvalue ratio; the bound is 100 x
that, 1e-10.  Class labels are compared with no cluster left out: each test first asserts that every cluster of the
restatement keeps |linearity - wal_lin_max| > 1e-8, so a 1e-10 difference cannot flip a class."""
import functools
import importlib

import numpy as np
import pytest

import scan_cluster_ref as R
from conftest import PKG, assert_bitwise

pytestmark = pytest.mark.gpu

LIN_TOL = 1e-10
LIN_MARGIN = 1e-8


def _yaw_pose(x, y, yaw):
    return [x, y, 0.0, 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]


@functools.lru_cache(maxsize=None)
def known_scans(n):
    """3 scans of n beams: a constant ring (one cluster closing on itself), arcs meeting across the seam with 1-2-beam
    specks and NaN / inf holes inside them, and jittered arcs at random places (every wave boundary gets crossed)."""
    amin, ainc = float(np.float32(-np.pi)), float(np.float32(2 * np.pi / n))
    rr = np.float32(0.1 / (2 * np.sin(np.pi / n)))  # neighbours on a ring of this radius are 0.1 m apart
    rng = np.random.default_rng(100 + n)
    r = np.full((3, n), np.inf, np.float32)
    r[0] = rr
    a, b = max(n // 8, 3), n // 2
    r[1, :a] = rr
    r[1, n - a:] = rr
    r[1, b:b + max(n // 4, 3)] = rr
    r[1, b + 1] = np.nan  # a hole inside a cluster: the link skips it
    r[1, a + 1] = rr * np.float32(2.0)  # a 1-beam speck
    r[1, a + 3:a + 5] = rr * np.float32(3.0)  # a 2-beam speck
    r[1, n - a - 2] = -np.inf
    i = 0
    while i < n:  # random arcs, lengths 1 .. 40, radii rr * (0.5 .. 1.5), gaps 0 .. 3 beams
        m = int(rng.integers(1, 41))
        r[2, i:i + m] = rr * np.float32(rng.uniform(0.5, 1.5)) * (1 + rng.normal(0, 0.01, min(m, n - i))).astype(
            np.float32)
        i += m + int(rng.integers(0, 4))
    r[2, rng.random(n) < 0.05] = np.nan
    poses = np.array([_yaw_pose(0.0, 0.0, 0.0), _yaw_pose(1.5, -2.0, 0.7), _yaw_pose(-3.0, 0.25, -2.9)])
    return r, poses, amin, ainc, 50.0


@functools.lru_cache(maxsize=None)
def batch(n_scans, n_beams):
    synth = importlib.import_module(PKG + ".synth")
    real, virt, poses, _, amin, ainc, rmax = synth.laser_scan_batch(n_scans, n_beams)
    return real, virt, poses, amin, ainc, rmax


@functools.lru_cache(maxsize=None)
def reference(kind, a, b, min_cluster_points=1):
    """the restatement of every scan of a case, computed once: (list of ScanClusters, beam directions)"""
    if kind == "known":
        r, poses, amin, ainc, rmax = known_scans(a)
    else:
        r, _, poses, amin, ainc, rmax = batch(a, b)
    d = R.beam_dirs(r.shape[1], amin, ainc)
    p = R.ClusterParams(min_cluster_points=min_cluster_points)
    return [R.cluster_scan(r[s], d, rmax, poses[s], p) for s in range(r.shape[0])], d


def _meta(cd, amin, ainc, rmax):
    return cd.LaserScan(ranges=None, angle_min=amin, angle_increment=ainc, range_max=rmax)


def _check_clusters(res, refs, what):
    lin = np.concatenate([c.linearity for c in refs]) if refs else np.zeros(0)
    if lin.size:  # the precondition of the class comparison
        assert np.abs(lin - float(np.float32(0.001))).min() > LIN_MARGIN, f"{what}: a cluster sits on wal_lin_max"
    for s, c in enumerate(refs):
        w = f"{what} scan {s}"
        assert int(res.n_clusters[s]) == c.n_clusters, f"{w}: n_clusters {res.n_clusters[s]} != {c.n_clusters}"
        assert_bitwise(res.beam_cluster[s], c.beam_cluster, w + " beam_cluster")
        assert_bitwise(res.beam_class[s], c.beam_class, w + " beam_class")
        assert_bitwise(res.beam_xy[s], c.beam_xy, w + " beam_xy")
        t = res.clusters[s]
        assert_bitwise(t["first_beam"], c.first_beam, w + " first_beam")
        assert_bitwise(t["n_points"], c.n_points, w + " n_points")
        assert_bitwise(t["length"], c.length, w + " length")
        assert_bitwise(t["cls"], c.cls, w + " class")
        if c.n_clusters:
            d = float(np.abs(t["linearity"] - c.linearity).max())
            assert d <= LIN_TOL, f"{w}: linearity differs by {d}"
        for k, got in ((R.WALL, res.wall_cloud(s)), (R.OBJECT, res.object_cloud(s)), (R.UNKNOWN, res.unknown_cloud(s))):
            assert_bitwise(got, c.clouds[k], f"{w} cloud of class {k}")


def _present(refs):
    cls = np.concatenate([c.cls for c in refs])
    return {k: int((cls == k).sum()) for k in (R.WALL, R.OBJECT, R.UNKNOWN)}, sum(c.merged for c in refs), \
        sum(c.ring for c in refs)


@pytest.mark.parametrize("min_cluster_points", [1, 3])
@pytest.mark.parametrize("n_beams", [16, 64, 65, 130])
def test_known_answer_scans(pkg, gpu, n_beams, min_cluster_points):
    cd = pkg.change_detection
    r, poses, amin, ainc, rmax = known_scans(n_beams)
    refs, _ = reference("known", n_beams, 0, min_cluster_points)
    assert refs[0].ring and refs[0].n_clusters == 1 and refs[1].merged  # what the scans were built to show
    res = cd.LidarClusterer(min_cluster_points=min_cluster_points).process(r, _meta(cd, amin, ainc, rmax), poses)
    _check_clusters(res, refs, f"{n_beams} beams, min {min_cluster_points}")


@pytest.mark.parametrize("n_scans,n_beams", [(32, 720), (8, 1440), (2, 4096)])
def test_synthetic_batches(pkg, gpu, n_scans, n_beams):
    """the change detector's scan batches; 4096 beams is the largest scan one workgroup stages (above 64 KiB of LDS)"""
    cd = pkg.change_detection
    real, _, poses, amin, ainc, rmax = batch(n_scans, n_beams)
    refs, _ = reference("batch", n_scans, n_beams)
    classes, merges, rings = _present(refs)
    assert all(v > 0 for v in classes.values()) and merges > 0, (classes, merges)
    if n_beams <= 1440:
        assert rings > 0
    res = cd.LidarClusterer().process(real, _meta(cd, amin, ainc, rmax), poses)
    _check_clusters(res, refs, f"{n_scans}x{n_beams}")


def test_device_tensor_input_and_identity_poses(pkg, gpu):
    """a device tensor is taken as it is; poses=None equals identity poses"""
    import torch

    cd = pkg.change_detection
    real, _, _, amin, ainc, rmax = batch(8, 1440)
    meta = _meta(cd, amin, ainc, rmax)
    a = cd.LidarClusterer().process(torch.from_numpy(real).cuda(), meta, None)
    ident = np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], (8, 1))
    b = cd.LidarClusterer().process(real, meta, ident)
    d = R.beam_dirs(1440, amin, ainc)
    _check_clusters(a, [R.cluster_scan(real[s], d, rmax, None) for s in range(8)], "poses=None")
    assert_bitwise(a.beam_xy, b.beam_xy, "beam_xy, None vs identity")
    assert_bitwise(a.beam_cluster, b.beam_cluster, "beam_cluster, None vs identity")
    for k in ("wall", "object", "unknown"):
        assert_bitwise(cd.D.to_host(getattr(a, k + "_xyz")), cd.D.to_host(getattr(b, k + "_xyz")), k + " cloud")
        assert_bitwise(getattr(a, k + "_offsets"), getattr(b, k + "_offsets"), k + " offsets")


def test_edge_cases(pkg, gpu):
    cd = pkg.change_detection
    meta = _meta(cd, -3.0, 0.1, 10.0)
    res = cd.LidarClusterer().process(np.zeros((0, 64), np.float32), meta)
    assert res.beam_cluster.shape == (0, 64) and res.clusters == [] and res.wall_offsets.tolist() == [0]
    r = np.full((2, 64), np.nan, np.float32)
    r[1, 10:14] = 0.5  # one scan of all NaN beside a scan with one small cluster
    res = cd.LidarClusterer().process(r, meta)
    assert res.n_clusters.tolist() == [0, 1] and (res.beam_cluster[0] == -1).all() and (res.beam_class[0] == 0).all()
    assert np.isnan(res.beam_xy[0]).all()
    assert res.object_offsets.tolist() == [0, 0, 4] and res.wall_offsets.tolist() == [0, 0, 0]
    assert res.object_cloud(0).shape == (0, 3) and res.object_cloud(1).shape == (4, 3)
    # an empty object list through the filter and the observations
    virt = np.full((2, 64), 2.0, np.float32)
    kept, off, mask = cd.ObjectMapFilter().process(np.zeros((0, 3), np.float32), [0, 0, 0], virt, meta)
    assert kept.shape[0] == 0 and off.tolist() == [0, 0, 0] and mask.size == 0
    assert [o.shape for o in cd.cluster_observations(np.zeros((0, 3), np.float32), [0, 0, 0])] == [(0, 5), (0, 5)]
    with pytest.raises(pkg._lib.OTError, match="4097"):
        cd.LidarClusterer().process(np.zeros((1, 4097), np.float32), meta)


@functools.lru_cache(maxsize=None)
def filtered_reference(n_scans, n_beams):
    """the restatement of the filter on the OBJECT clouds of a batch: (objects, offsets, masks, kept, kept offsets)"""
    _, virt, poses, amin, ainc, rmax = batch(n_scans, n_beams)
    refs, d = reference("batch", n_scans, n_beams)
    objs = [c.clouds[R.OBJECT] for c in refs]
    out = [R.object_map_filter(objs[s], virt[s], d, rmax, poses[s]) for s in range(n_scans)]
    off = np.concatenate([[0], np.cumsum([o.shape[0] for o in objs])]).astype(np.int64)
    koff = np.concatenate([[0], np.cumsum([k.shape[0] for _, k in out])]).astype(np.int64)
    return np.concatenate(objs), off, np.concatenate([m for m, _ in out]), np.concatenate([k for _, k in out]), koff


@pytest.mark.parametrize("n_scans,n_beams", [(32, 720), (8, 1440)])
def test_object_map_filter(pkg, gpu, n_scans, n_beams):
    """the added boxes stand >= 1.5 m from every saved wall (kept); the surviving pillars coincide with saved ones
    (removed)"""
    cd = pkg.change_detection
    _, virt, poses, amin, ainc, rmax = batch(n_scans, n_beams)
    obj, off, mask, kept, koff = filtered_reference(n_scans, n_beams)
    assert mask.any() and not mask.all(), "the restatement must both keep and remove points"
    got, goff, gmask = cd.ObjectMapFilter(0.5).process(obj, off, virt, _meta(cd, amin, ainc, rmax), poses)
    assert_bitwise(gmask, mask.astype(np.uint8), "keep mask")
    assert_bitwise(goff, koff, "kept offsets")
    assert_bitwise(cd.D.to_host(got), kept, "kept points")
    # chained on the device: the clusterer's object cloud goes in as the tensor it is
    real = batch(n_scans, n_beams)[0]
    res = cd.LidarClusterer().process(real, _meta(cd, amin, ainc, rmax), poses)
    got2, goff2, _ = cd.ObjectMapFilter(0.5).process(res.object_xyz, res.object_offsets, virt,
                                                     _meta(cd, amin, ainc, rmax), poses)
    assert_bitwise(goff2, koff, "kept offsets (chained)")
    assert_bitwise(cd.D.to_host(got2), kept, "kept points (chained)")


def test_object_map_filter_scan_without_walls(pkg, gpu):
    cd = pkg.change_detection
    meta = _meta(cd, -3.0, 0.1, 10.0)
    virt = np.full((2, 64), np.inf, np.float32)
    virt[1, 30] = 2.0
    obj = np.array([[5.0, 5.0, 0.1], [6.0, 5.0, 0.2], [5.0, 5.0, 0.3]], np.float32)
    kept, off, mask = cd.ObjectMapFilter().process(obj, [0, 2, 3], virt, meta)
    assert mask.tolist() == [0, 0, 1] and off.tolist() == [0, 0, 1]  # :93 — no wall points, nothing published
    assert_bitwise(cd.D.to_host(kept), obj[2:], "kept point keeps its z")


def test_cluster_observations(pkg, gpu):
    cd = pkg.change_detection
    _, _, _, kept, koff = filtered_reference(32, 720)
    t = np.linspace(0, 1, 12)
    thin = np.stack([5 + 0.3 * t, np.zeros(12), np.zeros(12)], axis=1)  # 12 points, no thickness
    short = np.array([[9.0, 9.0, 0.0], [9.1, 9.3, 0.0], [9.3, 9.1, 0.0]])  # 3 points
    wide = np.stack([20 + 0.3 * t, 0.3 * np.sin(7 * t) ** 2, np.zeros(12)], axis=1)
    hand = np.concatenate([thin, short, wide]).astype(np.float32)
    pts = np.concatenate([kept, hand])
    off = np.concatenate([koff, [koff[-1] + hand.shape[0]]])
    poses = np.array([_yaw_pose(0.1 * j, -0.2 * j, 0.3 * j) for j in range(off.size - 1)])
    want = [R.cluster_observations(pts[off[j]:off[j + 1]], poses[j]) for j in range(off.size - 1)]
    assert sum(w[0].shape[0] for w in want[:-1]) > 0, "the filtered objects must give an observation"
    assert want[-1][0].shape[0] == 1 and want[-1][1] == 1 and want[-1][2] == 1  # hand-made: one kept, one per rule
    assert sum(w[1] for w in want) > 0 and sum(w[2] for w in want) > 0
    got = cd.cluster_observations(pts, off, poses)
    for j, (g, w) in enumerate(zip(got, want)):
        assert_bitwise(g, w[0], f"observations of cloud {j}")
    # xy-only input and no pose
    got = cd.cluster_observations(np.ascontiguousarray(hand[:, :2]), [0, hand.shape[0]])
    assert_bitwise(got[0], R.cluster_observations(hand)[0], "observations of xy input")
