"""The numpy statement of FPFH and of the feature matcher (tests/fpfh_ref.py) against known answers, and the properties
the designed clouds of tests/fpfh_clouds.py were designed for.  No device."""
import numpy as np
import pytest

import fpfh_clouds as FC
import fpfh_ref as FR
from conftest import assert_bitwise

ALL = sorted(FC.cases())


def _hist(*bins_):
    h = np.zeros(33)
    for b in bins_:
        h[b] = 100.0
    return h


def test_planar_grid_known_answer():
    """All normals (0, 0, 1) and every dp in the plane: a1 = a2 = 0 (no swap, f3 = 0), v is a unit vector in the plane
    (f2 = 0) and f1 = atan2(0, 1) = 0, so every pair lands in bins 5, 16 and 27.  With k = 11 the increment is 10.0
    and ten additions give exactly 100.  FPFH: the block sum and the bin accumulate the same values (the other bins
    add +0), so the bin is x (100 / x) + 100 with x (100 / x) within one ulp of 100: 200 within 4 ulp."""
    P, N = FC.planar()
    ref = FR.compute(P, N, 11)
    assert not ref["spfh_fragile"].any() and not ref["fpfh_fragile"].any()
    assert_bitwise(ref["spfh"], np.broadcast_to(_hist(5, 16, 27), (len(P), 33)), "planar SPFH")
    F = ref["fpfh"]
    on = np.zeros(33, bool)
    on[[5, 16, 27]] = True
    assert (F[:, ~on] == 0).all()
    assert (np.abs(F[:, on] - 200.0) <= 4 * np.spacing(200.0)).all()


def test_pair_no_swap():
    """n1 = (0.6, 0, 0.8), dp = (1, 0, 0), n2 = (0, 0, 1): a1 = 0.6, a2 = 0, acos(0.6) < acos(0): no swap, f3 = a1.
    v = dp x n1 = (0, -0.8, 0) -> (0, -1, 0); w = n1 x v = (0.8, 0, -0.6); f2 = v.n2 = 0; f1 = atan2(-0.6, 0.8)."""
    f, close = FR.pair_features([0, 0, 0], [0.6, 0, 0.8], [[1.0, 0, 0]], [[0, 0, 1.0]])
    assert not close.any()
    assert f[0, 1] == 0.0 and f[0, 2] == 0.6
    assert abs(f[0, 0] - (-np.arctan2(0.6, 0.8))) <= 2 * np.spacing(0.7)
    assert FR.bins(FR.bin_coordinates(f)).tolist() == [[4, 5, 8]]  # 11 (pi - 0.6435) / 2 pi = 4.37; 5.5; 8.8


def test_pair_swap():
    """n1 = (0, 0, 1), dp = (1, 0, 0), n2 = (0.6, 0, 0.8): a1 = 0, a2 = 0.6, acos(0) > acos(0.6): swap, so
    n1 = (0.6, 0, 0.8), n2 = (0, 0, 1), dp = (-1, 0, 0), f3 = -0.6.  v = dp x n1 = (0, 0.8, 0) -> (0, 1, 0);
    w = n1 x v = (-0.8, 0, 0.6); f2 = 0; f1 = atan2(0.6, 0.8)."""
    f, close = FR.pair_features([0, 0, 0], [0, 0, 1.0], [[1.0, 0, 0]], [[0.6, 0, 0.8]])
    assert not close.any()
    assert f[0, 1] == 0.0 and f[0, 2] == -0.6
    assert abs(f[0, 0] - np.arctan2(0.6, 0.8)) <= 2 * np.spacing(0.7)
    assert FR.bins(FR.bin_coordinates(f)).tolist() == [[6, 5, 2]]  # 6.63; 5.5; 2.2


def test_pair_zero_returns():
    f, _ = FR.pair_features([1.0, 2.0, 3.0], [0, 0, 1.0], [[1.0, 2.0, 3.0]], [[0.6, 0, 0.8]])  # coincident points
    assert_bitwise(f, np.zeros((1, 3)), "coincident points")
    f, _ = FR.pair_features([0, 0, 0], [1.0, 0, 0], [[2.0, 0, 0]], [[0, 1.0, 0]])  # dp parallel to n1: dp x n1 = 0
    assert_bitwise(f, np.zeros((1, 3)), "dp parallel to n1")
    assert FR.bins(FR.bin_coordinates(f)).tolist() == [[5, 5, 5]]  # a zero pair: bins 5, 16 and 27


def test_two_point_clouds():
    P = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    ref = FR.compute(P, np.array([[0.6, 0, 0.8], [0, 0, 1.0]]), 2)
    assert [l.tolist() for l, _ in ref["lists"]] == [[0, 1], [1, 0]]
    assert_bitwise(ref["spfh"][0], _hist(4, 16, 30), "the no-swap pair")
    # seen from point 1: dp = (-1, 0, 0), a1 = 0, a2 = -0.6: the swap, f3 = 0.6, and the same frame as from point 0
    assert_bitwise(ref["spfh"][1], _hist(4, 16, 30), "the swapped pair")
    # one neighbour at d2 = 1: the neighbour's row over 1, scaled to sum 100, plus the own row
    assert_bitwise(ref["fpfh"], np.broadcast_to(_hist(4, 16, 30) * 2, (2, 33)), "two-point FPFH")
    same = FR.compute(np.zeros((2, 3)), np.array([[0.6, 0, 0.8], [0, 0, 1.0]]), 2)
    assert [l.tolist() for l, _ in same["lists"]] == [[0, 1], [0, 1]]  # point 1 skips entry 0 and pairs with itself
    assert_bitwise(same["spfh"], np.broadcast_to(_hist(5, 16, 27), (2, 33)), "coincident SPFH")
    assert_bitwise(same["fpfh"], same["spfh"], "d2 == 0 is skipped: FPFH = 0 * 0 + SPFH")
    one = FR.compute(np.zeros((1, 3)), np.array([[0, 0, 1.0]]), 5)
    assert_bitwise(one["spfh"], np.zeros((1, 33)), "n = 1 SPFH")
    assert_bitwise(one["fpfh"], np.zeros((1, 33)), "n = 1 FPFH")


@pytest.mark.parametrize("name", ALL)
def test_block_sums_and_fragile_cap(name):
    """Each SPFH block is len - 1 additions of 100 / (len - 1): at most 128 roundings of 2^-53 relative on values up
    to 100, so within 1.5e-12 of 100.  An FPFH block is 100 (sum of the weighted bins) / (their sum, accumulated in
    another order) + 100: the two orders differ by at most 2 x 127 x 11 roundings, 3.1e-13 relative, so within 1e-10
    of 200.  The designed clouds have generic normals: none of their points may be fragile."""
    ref = FC.reference(name)
    S, F = ref["spfh"], ref["fpfh"]
    lens = np.array([len(l) for l, _ in ref["lists"]])
    far = np.array([len(l) > 1 and bool((d[1:] != 0).any()) for l, d in ref["lists"]])
    sb, fb = S.reshape(-1, 3, 11).sum(axis=2), F.reshape(-1, 3, 11).sum(axis=2)
    assert (np.abs(sb[lens > 1] - 100.0) <= 1.5e-12).all()
    assert (sb[lens <= 1] == 0).all() and (fb[lens <= 1] == 0).all()
    assert (np.abs(fb[far] - 200.0) <= 1e-10).all()
    assert np.isfinite(F).all() and (F >= 0).all()
    nf = int(ref["fpfh_fragile"].sum())
    print(f"{name}: {len(S)} points, lists of {lens.min()}..{lens.max()}, {nf} fragile")
    assert nf == 0 and not ref["spfh_fragile"].any()


def test_designed_properties():
    lens = np.array([len(l) for l, _ in FC.reference("sphere_hybrid_k100")["lists"]])
    assert lens.max() > 64 and (lens <= 64).any() and len(set(lens.tolist())) > 10  # mixed, on both sides of 64
    for k in (64, 65, 128):
        assert all(len(l) == k for l, _ in FC.reference(f"random_k{k}")["lists"])
    co = FC.reference("coincident_k9")["lists"]
    assert any(l[0] != i for i, (l, _) in enumerate(co))  # entry 0 is not the query
    assert all((d[:4] == 0).all() and (d[4:] > 0).all() for _, d in co)
    far = FC.reference("far_point_hybrid_k16")
    assert far["lists"][100][0].tolist() == [100]
    assert (far["spfh"][100] == 0).all() and (far["fpfh"][100] == 0).all()
    lat = FC.reference("lattice_k27")["lists"]
    assert sum(len(set(d.tolist())) < len(d) for _, d in lat) == len(lat)  # distance ties in every list
    assert all(len(l) == 5 for l, _ in FC.reference("n5_k20")["lists"])


def test_the_fragile_flag_works():
    """Exact radial normals on a sphere: |a1| = |a2| up to rounding, so the swap is decided by the last bits of two
    acos values.  A lattice of spacing 0.1 (coordinates rounded) with normals along the axes: |dx| and |dy| of a
    diagonal offset differ in their last bits, the same tie."""
    S, SN = FC.sphere()
    ref = FR.compute(S, SN, 100, 0.06)
    assert ref["spfh_fragile"].mean() > 0.5 and (ref["fpfh_fragile"] >= ref["spfh_fragile"]).all()
    L = FC.lattice(5, 0.1)
    axes = np.eye(3)[np.arange(len(L)) % 3]
    lat = FR.compute(L, axes, 27)
    assert lat["spfh_fragile"].any() and lat["fpfh_fragile"].sum() >= lat["spfh_fragile"].sum()
    # (a): a bin coordinate next to an integer: f3 = 6 / 11 - 1 + 1e-12 puts the third coordinate 5.5e-12 above 3
    f = np.array([[0.0, 0.0, 2 * 3.0 / 11 - 1 + 1e-12]])
    c = FR.bin_coordinates(f)
    assert abs(c[0, 2] - 3.0) < FR.FRAGILE_EPS and abs(c[0, 0] - 5.5) < 1e-12


def test_matcher_reference():
    tgt = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [5.0, 5.0]])
    src = np.array([[0.9, 0.0], [0.5, 0.0], [4.0, 4.0], [1.0, 0.1]])
    assert FR.nearest(src, tgt).tolist() == [1, 0, 3, 1]  # ties (0.5 between 0 and 1; rows 1 and 2): the lowest index
    pairs, fell = FR.correspondences(src, tgt)
    assert pairs.tolist() == [[0, 1], [1, 0], [2, 3], [3, 1]] and not fell
    # the targets' matches are 1, 0, 0, 2: source 3's target (1) prefers source 0, the other three pairs agree
    pairs, fell = FR.correspondences(src, tgt, True, 0.75)
    assert pairs.tolist() == [[0, 1], [1, 0], [2, 3]] and not fell  # 3 >= 0.75 x 4
    pairs, fell = FR.correspondences(src, tgt, True, 0.8)
    assert len(pairs) == 4 and fell  # 3 < 3.2: all pairs
