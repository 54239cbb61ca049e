"""GPU parity of correspondences_from_features (csrc/features.hip: the exhaustive sweep, its split over workgroups and
the mutual filter) with the exhaustive numpy matcher of tests/fpfh_ref.py: the pairs must be equal."""
import ctypes as C

import numpy as np
import pytest

import fpfh_clouds as FC
import fpfh_ref as FR

pytestmark = pytest.mark.gpu

WORKGROUP = 64                 # csrc/features.hip: query rows per workgroup
TILE_SMALL, TILE_LARGE = 64, 32  # ... and target rows per LDS tile for dim <= 33 and dim <= 128


def _match(pkg, src, tgt, mutual=False, ratio=0.1):
    """(pairs [k][2], fell_back) through the C ABI; src / tgt: [n][dim] / [m][dim]"""
    D, L = pkg._device, pkg._lib
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    n, m, dim = len(src), len(tgt), src.shape[1]
    corr = D.empty((n, 2), "int32")
    corr.fill_(-7)
    k, fell = C.c_int64(-1), C.c_int32(-1)
    d_src, d_tgt = D.to_device(src), D.to_device(tgt)
    L.call("ot_correspondences_from_features", D.ptr(d_src), n, D.ptr(d_tgt), m, dim, 1 if mutual else 0,
           float(ratio), D.ptr(corr), C.byref(k), C.byref(fell), D.stream_ptr())
    return D.to_host(corr)[:k.value], bool(fell.value)


def _check(pkg, src, tgt, mutual=False, ratio=0.1):
    got, fell = _match(pkg, src, tgt, mutual, ratio)
    want, wfell = FR.correspondences(src, tgt, mutual, ratio)
    assert got.shape == want.shape and fell == wfell
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} pairs differ, first {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"
    return got, fell


def _random(n, m, dim, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, dim)) * 100.0, rng.random((m, dim)) * 100.0


@pytest.mark.parametrize("n,m,dim", [(1500, 1300, 33), (300, 200, 1), (300, 200, 128), (200, 300, 34),
                                     (3000, 6000, 5),  # several tiles per split
                                     (1, 500, 33), (500, 1, 33), (1, 1, 33), (1, 1, 128)])
def test_random_columns(pkg, gpu, n, m, dim):
    src, tgt = _random(n, m, dim, n + m + dim)
    _check(pkg, src, tgt)
    _check(pkg, src, tgt, True, 0.0)


@pytest.mark.parametrize("n", [WORKGROUP - 1, WORKGROUP, WORKGROUP + 1])
@pytest.mark.parametrize("dim,tile", [(33, TILE_SMALL), (128, TILE_LARGE)])
def test_tile_and_workgroup_edges(pkg, gpu, n, dim, tile):
    for m in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
        src, tgt = _random(n, m, dim, 1000 * n + m)
        _check(pkg, src, tgt)
        _check(pkg, tgt, src, True, 0.0)


def test_ties_resolve_to_the_lowest_index(pkg, gpu):
    src, base = _random(400, 150, 33, 5)
    tgt = np.concatenate([base, base[::-1], base])  # every target three times
    got, _ = _check(pkg, src, tgt)
    assert (got[:, 1] < 150).all()
    same = np.broadcast_to(src[0], (300, 33))
    got, _ = _check(pkg, src[:70], same)
    assert (got[:, 1] == 0).all()
    got, fell = _check(pkg, same[:130], same, True, 0.0)  # all identical: only (0, 0) is mutual
    assert got.tolist() == [[0, 0]] and not fell


def test_fpfh_of_the_planar_cloud(pkg, gpu):
    """every column of the planar cloud's FPFH is the same histogram (200 in bins 5, 16 and 27): all matches are 0"""
    g, r = pkg.geometry, pkg.pipelines.registration
    P, N = FC.planar()
    pcd = g.PointCloud()
    pcd.points, pcd.normals = pkg.utility.Vector3dVector(P), pkg.utility.Vector3dVector(N)
    f = r.compute_fpfh_feature(pcd, g.KDTreeSearchParamKNN(11))
    corr = np.asarray(r.correspondences_from_features(f, f))
    F = f.data.T
    assert (F == F[0]).all()
    want, _ = FR.correspondences(F, F)
    assert corr.dtype == np.int32 and corr.tolist() == want.tolist()
    assert (corr[:, 1] == 0).all() and corr[:, 0].tolist() == list(range(len(P)))
    mutual = r.correspondences_from_features(f, f, mutual_filter=True, mutual_consistency_ratio=0.0)
    assert isinstance(mutual, pkg.utility.Vector2iVector) and np.asarray(mutual).tolist() == [[0, 0]]


@pytest.mark.parametrize("kept,fell_back", [(2, True), (3, False), (4, False)])
def test_mutual_filter_threshold(pkg, gpu, kept, fell_back):
    """12 sources on a line, `kept` targets next to sources picked by a permutation: exactly those pairs are mutual
    (every other source matches a target that prefers its own source).  ratio x n = 0.25 x 12 = 3 exactly."""
    src = np.stack([np.arange(12) * 10.0, np.zeros(12)], axis=1)
    pick = np.random.default_rng(kept).permutation(12)[:kept]
    tgt = src[pick] + np.array([0.0, 0.5])
    got, fell = _check(pkg, src, tgt, True, 0.25)
    assert fell == fell_back
    if fell_back:
        assert len(got) == 12 and got[:, 0].tolist() == list(range(12))
    else:
        order = np.argsort(pick)
        assert got.tolist() == [[int(pick[j]), int(j)] for j in order]
    plain, fell = _check(pkg, src, tgt, False, 0.25)
    assert len(plain) == 12 and not fell


def test_repeat_run_is_identical(pkg, gpu):
    src, tgt = _random(1500, 1300, 33, 77)
    a, b = _match(pkg, src, tgt, True, 0.0), _match(pkg, src, tgt, True, 0.0)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1]
