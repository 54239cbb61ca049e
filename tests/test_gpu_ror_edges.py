"""GPU parity at the edges of remove_radius_outlier (k_ror in csrc/outlier.hip over the grid of csrc/grid.h) against
the exhaustive float64 count of tests/ror_ref.py: kept indices, bit for bit.  Every cloud has at most 5 000 points.

* pairs a hair under the radius apart whose computed grid cells differ by 2 (found by a search on the CPU);
* separations exactly equal to the radius (strict <) and one double below it;
* coincident points, clusters of exactly nb_points and nb_points + 1;
* n = 1, 2, nb_points >= n, lines, a plane, one cell, 256 / 257 points, coordinates far from zero;
* the refusal of a grid that would be too large, and the call after it.
"""
import numpy as np
import pytest

import ror_ref as R
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu


def _ror_gpu(pkg, pts, nb, r):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.ascontiguousarray(pts, np.float64))
    out, idx = p.remove_radius_outlier(nb, r)
    idx = np.asarray(idx, np.int64).reshape(-1)
    assert_bitwise(np.asarray(out.points).reshape(-1, 3), np.asarray(pts, np.float64)[idx], "ROR selected points")
    return idx


def _check(pkg, pts, nb, r, what):
    assert len(pts) <= 5000
    ref = R.remove_radius_outlier(pts, nb, r)
    assert_bitwise(_ror_gpu(pkg, pts, nb, r), ref, what)
    return ref


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ror_cell_straddle(pkg, gpu, axis):
    """Pairs closer than the radius whose cells, computed as the grid computes them with cells of exactly the radius
    (floor((v - o) / r), o the cloud minimum), differ by 2, laid along one axis with 4 r between pairs: each point's
    only neighbour is its partner, nb_points = 1, so a partner the 3x3x3 block does not reach drops both points.

    The search (tests/ror_ref.py straddle_pairs; 9 900 faces per (o, r), the doubles within 6 steps of each face and
    of the point one radius on, r in 0.1, 0.02, 0.016, 2^-4, o in 0, -73, -1000.123, -3000.7, 517.77 radii, points
    100 .. 10 000 radii above o) FINDS such pairs: 0.1: 92 / 1376 / 1614 / 305 for the four non-zero origins,
    0.02: 61 / 1064 / 2800 / 0, 0.016: 32 / 1320 / 1692 / 0, none for o = 0 and none for the dyadic radius.  A
    library whose ROR grid has cells of exactly the radius drops every one of these pairs (as the oracle did); the
    grid's cells are therefore a factor 1 + 2^-20 wider than the radius (csrc/grid.h ROR_CELL_SCALE).  The clouds
    also carry the nearest misses: cells one apart, separation within 4 doubles of the radius on either side."""
    found = R.straddle_pairs(1.0)
    assert sum(len(miss) for o, r, miss, near in found) > 0, "the search found no cell-straddling pair"
    ran = 0
    for o, r, miss, near in found:
        if len(miss) == 0 and len(near) == 0:
            continue
        pairs = np.concatenate([miss[:400], near[:200]])
        pts = R.pair_cloud(o, r, pairs, axis)
        ref = _check(pkg, pts, 1, r, f"ROR kept, straddling pairs along axis {axis} (o = {o}, r = {r})")
        n_miss = min(len(miss), 400)
        assert ref[:2 * n_miss].tolist() == list(range(1, 2 * n_miss + 1))  # every such pair is a pair of neighbours
        ran += n_miss
    assert ran > 2000


@pytest.fixture(scope="module")
def lattice():
    g = np.stack(np.meshgrid(np.arange(-3, 5), np.arange(-3, 4), np.arange(-2, 4), indexing="ij"), -1)
    return g.reshape(-1, 3).astype(np.float64)  # 8 x 7 x 6


@pytest.mark.parametrize("nb", [1, 3, 4, 5, 6, 7])
def test_ror_exactly_on_radius(pkg, gpu, lattice, nb):
    """An integer lattice scaled by the dyadic r = 2^-4: axis neighbours are at exactly r (d2 == r r, excluded by the
    strict <), face diagonals beyond, so every count is 1.  With the radius one double above r the six axis
    neighbours count: 7 inside, 6 / 5 / 4 on faces / edges / corners.  nb_points runs over those counts.  The same
    lattice scaled by nextafter(r, 0) with radius r (coordinates are rounded products, so which neighbours fall
    inside is the reference's to say)."""
    r = 2.0 ** -4
    pts = lattice * r
    cnt = R.neighbour_counts(pts, r)
    assert (cnt == 1).all()
    assert len(_check(pkg, pts, nb, r, f"ROR({nb}) lattice at exactly r")) == 0
    up = float(np.nextafter(r, 1.0))
    cnt = R.neighbour_counts(pts, up)
    assert sorted(set(cnt.tolist())) == [4, 5, 6, 7] and (cnt == 7).sum() == 6 * 5 * 4
    ref = _check(pkg, pts, nb, up, f"ROR({nb}) lattice, radius one double above the spacing")
    assert len(ref) == int((cnt > nb).sum())
    below = lattice * float(np.nextafter(r, 0.0))
    cnt = R.neighbour_counts(below, r)
    assert cnt.max() == 7 and cnt.min() >= 1
    _check(pkg, below, nb, r, f"ROR({nb}) lattice scaled one double below r")


def test_ror_coincident_points(pkg, gpu):
    """Clusters of 1, nb, nb + 1 and nb + 2 identical points (count == cluster size: nb is dropped, nb + 1 kept) at
    the origin, at negative and at large (+-10^3) coordinates, 10 apart."""
    nb, r = 5, 0.05
    rng = np.random.default_rng(21)
    places = np.array([[0.0, 0.0, 0.0], [-1000.0, 3.0, 7.0], [1000.0, -1000.0, 0.5], [12.3, 1000.0, -1000.0]])
    parts, sizes = [], []
    for a, base in enumerate(places):
        for b, m in enumerate((1, nb, nb + 1, nb + 2)):
            parts.append(np.repeat((base + [10.0 * b, 0.0, 0.0])[None], m, 0))
            sizes += [m] * m
    perm = rng.permutation(len(sizes))
    pts = np.concatenate(parts)[perm]
    sizes = np.array(sizes)[perm]
    ref = _check(pkg, pts, nb, r, "ROR kept, coincident clusters")
    assert_bitwise(ref, np.nonzero(sizes > nb)[0], "clusters above nb_points kept, the others dropped")


def test_ror_small_n(pkg, gpu):
    one = np.array([[0.3, -0.2, 5.0]])
    assert len(_check(pkg, one, 1, 0.1, "ROR n = 1")) == 0
    two = np.array([[0.3, -0.2, 5.0], [0.3, -0.25, 5.0]])
    assert _check(pkg, two, 1, 0.1, "ROR n = 2, neighbours").tolist() == [0, 1]
    assert len(_check(pkg, two, 2, 0.1, "ROR n = 2, nb_points = n")) == 0
    assert len(_check(pkg, two, 1, 0.04, "ROR n = 2, apart")) == 0
    rng = np.random.default_rng(22)
    blob = rng.uniform(-0.01, 0.01, (50, 3)) - 3.0  # every point within r of every other: all counts are 50
    assert len(_check(pkg, blob, 49, 0.1, "ROR nb_points = n - 1")) == 50
    assert len(_check(pkg, blob, 50, 0.1, "ROR nb_points = n")) == 0
    assert len(_check(pkg, blob, 1000, 0.1, "ROR nb_points > n")) == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ror_line(pkg, gpu, axis):
    """two axes of extent 0 (one cell across): a line of 700 points with uneven gaps, at a negative offset"""
    rng = np.random.default_rng(23 + axis)
    pts = np.full((700, 3), -7.25)
    pts[:, axis] = np.cumsum(rng.uniform(0.002, 0.03, 700)) - 4.0
    ref = _check(pkg, pts[rng.permutation(700)], 4, 0.05, f"ROR kept, line along axis {axis}")
    assert 0 < len(ref) < 700


@pytest.mark.parametrize("flat", [0, 1, 2])
def test_ror_plane(pkg, gpu, flat):
    rng = np.random.default_rng(26 + flat)
    pts = rng.uniform(-1.0, 1.0, (3000, 3))
    pts[:, flat] = 2.5
    ref = _check(pkg, pts, 9, 0.06, f"ROR kept, plane of constant axis {flat}")
    assert 0 < len(ref) < 3000


def test_ror_one_cell_and_far_from_zero(pkg, gpu):
    """all points inside one cell (extent 0.9 r: counts still differ), then a sheet 10^4 radii from zero on every axis"""
    rng = np.random.default_rng(29)
    r = 0.1
    cube = rng.uniform(0.0, 0.9 * r, (500, 3)) + [4.0, -4.0, 0.0]
    cnt = R.neighbour_counts(cube, r)
    nb = int(np.median(cnt))
    ref = _check(pkg, cube, nb, r, "ROR kept, one cell")
    assert 0 < len(ref) < 500
    sheet = np.stack([rng.uniform(0, 1, 4000), rng.uniform(0, 1, 4000), rng.normal(0, 0.005, 4000)], 1)
    for shift in ([1234.5, -987.25, 4321.125], [-1000.1, -1000.2, -1000.3]):
        ref = _check(pkg, sheet + shift, 6, 0.03, f"ROR kept, sheet shifted by {shift}")
        assert 0 < len(ref) < 4000


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_ror_launch_tail(pkg, gpu, n):
    rng = np.random.default_rng(n)
    pts = rng.normal(0, 0.05, (n, 3))
    ref = _check(pkg, pts, 8, 0.03, f"ROR kept, {n} points")
    assert 0 < len(ref) < n


def test_ror_grid_refusal_leaves_no_state(pkg, gpu):
    """two points 2 x 10^6 radii apart need more cells per axis than the grid allows: refused through the facade;
    the next call is unaffected"""
    r = 0.01
    rng = np.random.default_rng(31)
    cloud = rng.normal(0, 0.03, (1000, 3))
    before = _check(pkg, cloud, 5, r, "ROR kept before the refusal")
    far = np.array([[0.0, 0.0, 0.0], [2.0e6 * r, 0.0, 0.0]])
    with pytest.raises(RuntimeError, match="neighbour grid out of range"):
        _ror_gpu(pkg, far, 1, r)
    with pytest.raises(RuntimeError, match="neighbour grid out of range"):
        _ror_gpu(pkg, far[:, [2, 1, 0]], 1, r)
    after = _check(pkg, cloud, 5, r, "ROR kept after the refusal")
    assert_bitwise(after, before, "same cloud, same answer")
    assert 0 < len(after) < 1000
