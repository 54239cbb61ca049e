"""The numpy references of the edge tests (tests/ror_ref.py, tests/voxel_diff_ref.py) pinned against the oracle, and
the cell-straddle search itself.  No GPU.

The exhaustive ROR reference also agrees with the oracle on the voxel-downsampled surface cloud of
test_gpu_filters.py (53 355 points, ROR(16, 0.05) keeps 52 150 and ROR(4, 0.02) 41 519, identical indices); that
run takes a minute of numpy and is not repeated here.
"""
import numpy as np
import pytest

import ror_ref as R
import voxel_diff_ref as V
from conftest import assert_bitwise


@pytest.fixture(scope="module")
def cloud():
    """a small cloud with structure at the scale of the radii used: a noisy sheet, a dense blob, a sparse halo, and
    coincident points; coordinates on both sides of zero"""
    rng = np.random.default_rng(11)
    sheet = np.stack([rng.uniform(-0.5, 0.5, 1500), rng.uniform(-0.5, 0.5, 1500), rng.normal(0, 0.004, 1500)], 1)
    blob = rng.normal(0, 0.03, (400, 3)) + [0.2, -0.1, 0.3]
    halo = rng.uniform(-1.5, 1.5, (300, 3))
    pts = np.concatenate([sheet, blob, halo, np.repeat(sheet[:3], 5, 0)])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


@pytest.mark.parametrize("nb,r", [(1, 0.02), (4, 0.05), (16, 0.1), (2300, 2.0)])
def test_ror_ref_matches_oracle(O, cloud, nb, r):
    ref = R.remove_radius_outlier(cloud, nb, r)
    assert_bitwise(ref, O.remove_radius_outlier(cloud, nb, r), f"ROR({nb}, {r}) reference vs oracle")
    if nb < 2300:
        assert 0 < len(ref) < len(cloud)  # the case decides something


def test_ror_ref_counts_by_hand():
    """self counts, the comparison is strict, coincident points count each other"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0], [-5, 0, 0]], np.float64)
    assert R.neighbour_counts(pts, 1.0).tolist() == [1, 2, 2, 1, 1]  # |0 - 1| == r: excluded
    assert R.neighbour_counts(pts, np.nextafter(1.0, 2.0)).tolist() == [3, 3, 3, 1, 1]
    assert R.remove_radius_outlier(pts, 1, 1.0).tolist() == [1, 2]
    with pytest.raises(RuntimeError):
        R.remove_radius_outlier(pts, 0, 1.0)


@pytest.mark.parametrize("origin", [(-2.0, -2.0, -2.0), (0.0, 0.0, 0.0), (0.013, -0.4, 0.25)])
def test_voxel_diff_ref_matches_oracle(O, cloud, origin):
    """origin below the clouds (no negative cell) and inside them (negative cells on every axis)"""
    rng = np.random.default_rng(12)
    new = cloud
    old = np.concatenate([cloud[:1200], cloud[1500:] + rng.normal(0, 0.02, (len(cloud) - 1500, 3))])
    ra, rr = V.voxel_key_diff(new, old, 0.05, origin)
    oa, orr = O.voxel_key_diff(new, old, 0.05, origin)
    assert len(ra) > 0 and len(rr) > 0
    if origin != (-2.0, -2.0, -2.0):
        assert (ra < 0).any() and (ra > 0).any()
    assert_bitwise(ra, oa, "added cells, reference vs oracle")
    assert_bitwise(rr, orr, "removed cells, reference vs oracle")
    # the multi form is the single form per object with the object in front
    ma, mr = V.voxel_key_diff_multi([new, np.zeros((0, 3)), old], [old, np.zeros((0, 3)), new], 0.05, origin)
    assert_bitwise(ma, np.concatenate([np.insert(oa, 0, 0, 1), np.insert(orr, 0, 2, 1)]), "multi added")
    assert_bitwise(mr, np.concatenate([np.insert(orr, 0, 0, 1), np.insert(oa, 0, 2, 1)]), "multi removed")


def test_voxel_diff_ref_order_is_signed():
    pts = np.array([[-0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5], [0.5, 0.5, 0.5], [-1.0, 0.0, 1.0]])
    a, r = V.voxel_key_diff(pts, np.zeros((0, 3)), 1.0, (0, 0, 0))
    assert a.tolist() == [[-1, 0, 0], [-1, 0, 1], [0, -1, 0], [0, 0, -1], [0, 0, 0]] and len(r) == 0
    assert a.dtype == np.int32


def test_straddle_search_finds_missed_neighbours(O):
    """What the search establishes.  With cells of exactly the radius anchored at the cloud minimum o, there ARE pairs
    with (v1 - v2)^2 < r r whose computed cells floor((v - o) / r) differ by 2: for every non-dyadic radius as soon as
    o lies a few radii below zero (v - o is then rounded at the spacing of v - o, coarser than the spacing of v that
    the separation is measured in), and for o above zero at r = 0.1.  None for o = 0 (v - o is exact) nor for the
    dyadic radius with o a multiple of a small power of two.  With cells wider by 2^-20 (csrc/grid.h ROR_CELL_SCALE)
    the same walk finds none, as the rounding bound there says.  The oracle, given such a cloud, keeps what the
    exhaustive count keeps."""
    found = R.straddle_pairs(1.0)
    assert len(found) == len(R.STRADDLE_RADII) * len(R.STRADDLE_ORIGINS)
    assert R.STRADDLE_FACES[1] - R.STRADDLE_FACES[0] >= 3000
    hits = {(round(o / r, 3), r): len(miss) for o, r, miss, near in found}
    print("pairs two cells apart yet closer than r, per (origin / r, r):", hits)
    for r in (0.1, 0.02, 0.016):
        assert hits[(-1000.123, r)] > 0 and hits[(-3000.7, r)] > 0
        assert hits[(0.0, r)] == 0
    for o, r, miss, near in found:
        if len(miss):
            d = miss[:, 1] - miss[:, 0]
            assert ((d * d) < r * r).all() and (R.cell_of(miss[:, 1], o, r) - R.cell_of(miss[:, 0], o, r) >= 2).all()
    assert all(len(miss) == 0 for o, r, miss, near in R.straddle_pairs(R.ROR_CELL_SCALE))
    o, r, miss, near = max(found, key=lambda f: len(f[2]))
    pts = R.pair_cloud(o, r, miss, 0, max_pairs=300)
    ref = R.remove_radius_outlier(pts, 1, r)
    assert ref.tolist() == list(range(1, len(pts)))  # every pair kept, the anchor dropped
    assert_bitwise(O.remove_radius_outlier(pts, 1, r), ref, "oracle ROR on cell-straddling pairs")
