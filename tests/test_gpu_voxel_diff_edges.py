"""GPU parity at the edges of voxel_key_diff / voxel_key_diff_multi (csrc/change.hip) against the set difference of
tests/voxel_diff_ref.py, bit for bit -- the multi form against an independent reference, not against the single form.

* negative lattice coordinates, points exactly on voxel faces and one double either side of them;
* key layouts that fill 64 bits (with and without an object field) and one that needs 65;
* field widths: an axis of extent 0, extents of 2^b - 1 and 2^b cells, object counts around powers of two, 2048 / 2049;
* set logic: permuted duplicates, disjoint and empty clouds, an object only in the old map, sizes around the sort tile;
* the range refusals of both forms (too far, NaN, inf) and the call after each.
"""
import numpy as np
import pytest

import voxel_diff_ref as V
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

E3 = np.zeros((0, 3))


def _single(pkg, new, old, vs, origin, what):
    a, r = pkg.change_detection.voxel_key_diff(new, old, vs, origin)
    ra, rr = V.voxel_key_diff(new, old, vs, origin)
    assert a.dtype == np.int32 and r.dtype == np.int32
    assert_bitwise(a.reshape(-1, 3), ra, f"{what}: added cells")
    assert_bitwise(r.reshape(-1, 3), rr, f"{what}: removed cells")
    return ra, rr


def _multi(pkg, news, olds, vs, origin, what):
    assert sum(len(c) for c in news) <= 5000 and sum(len(c) for c in olds) <= 5000
    a, r = pkg.change_detection.voxel_key_diff_multi(news, olds, vs, origin)
    ra, rr = V.voxel_key_diff_multi(news, olds, vs, origin)
    assert a.dtype == np.int32 and r.dtype == np.int32
    assert_bitwise(a.reshape(-1, 4), ra, f"{what}: added (object, cell)")
    assert_bitwise(r.reshape(-1, 4), rr, f"{what}: removed (object, cell)")
    return ra, rr


def _split(rng, pts, k):
    """pts dealt into k objects of uneven sizes"""
    cuts = np.sort(rng.integers(0, len(pts) + 1, k - 1))
    return np.split(pts, cuts)


# ------------------------------------------------------------------------------------------ negative coordinates
def test_diff_origin_inside_the_clouds(pkg, gpu):
    rng = np.random.default_rng(41)
    new = rng.uniform(-1.0, 1.0, (4000, 3))
    old = np.concatenate([new[:2500], rng.uniform(-1.0, 1.0, (1500, 3))])[rng.permutation(4000)]
    origin = (0.013, -0.21, 0.4)
    ra, rr = _single(pkg, new, old, 0.05, origin, "origin inside")
    assert (ra < 0).any(0).all() and (ra > 0).any(0).all() and len(rr) > 0  # both signs on every axis
    ma, mr = _multi(pkg, _split(rng, new, 3), _split(rng, old, 3), 0.05, origin, "origin inside, 3 objects")
    assert (ma[:, 1:] < 0).any(0).all() and len(mr) > 0


def test_diff_points_on_voxel_faces(pkg, gpu):
    """origin + k vs for k in -8 .. 8 with vs = 2^-5 and a dyadic origin (every face exactly representable), and the
    doubles one step below and above each face.  A face and the step above it are in cell k, for negative k as for
    positive; the step below is in cell k - 1 unless p - origin rounds back onto the face (it does where |p| < |origin|
    halves the spacing), which the reference decides with the same two rounded operations."""
    rng = np.random.default_rng(42)
    vs, origin = 2.0 ** -5, np.array([0.5, -1.25, 3.0])
    k = np.arange(-8, 9, dtype=np.float64)
    per_axis = []
    for a in range(3):
        face = origin[a] + k * vs
        per_axis.append(np.concatenate([face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf)]))
    c = V.cells(np.stack(per_axis, 1), vs, origin)
    assert (c[:17] == k[:, None]).all() and (c[34:] == k[:, None]).all()
    assert (c[17:34] == k[:, None] - 1).sum() > 17 and (c[17:34] == k[:, None]).sum() > 0  # both outcomes occur

    def draw(n):
        return np.stack([per_axis[a][rng.integers(0, 51, n)] for a in range(3)], 1)

    new, old = draw(2500), draw(2500)
    ra, rr = _single(pkg, new, old, vs, origin, "faces")
    assert ra.min() == -9 and ra.max() == 8 and len(rr) > 0  # -9: a step below face -8
    _multi(pkg, _split(rng, new, 4), _split(rng, old, 4), vs, origin, "faces, 4 objects")
    _single(pkg, new, E3, vs, origin, "faces vs empty")  # every occupied cell, none cancelled


# ------------------------------------------------------------------------------------------------ 64-bit layouts
def _cell_points(cells):
    return np.asarray(cells, np.float64) + 0.5  # voxel_size 1, origin 0: the middle of each cell


def test_multi_layout_fills_64_bits_without_object_field(pkg, gpu):
    """One object whose joint extents need 22 + 21 + 21 bits: the object field starts at bit 64.  The object column
    must be 0 and the cells right -- or the call refused as too large; never the key's low bits in the column."""
    new = _cell_points([[0, 0, 0], [(1 << 21) + 5, (1 << 20) + 3, (1 << 20) + 7], [-100, 17, -3]])
    old = _cell_points([[0, 0, 0], [7, (1 << 20) + 1, 5]])
    ext = np.concatenate([new, old]).max(0) - np.concatenate([new, old]).min(0)
    assert [int(e).bit_length() for e in ext] == [22, 21, 21]
    try:
        ra, rr = _multi(pkg, [new], [old], 1.0, (0, 0, 0), "22 + 21 + 21 bits, one object")
    except RuntimeError as e:
        assert "too large for 64-bit keys" in str(e)
    else:
        assert len(ra) == 2 and len(rr) == 1 and (ra[:, 0] == 0).all() and (rr[:, 0] == 0).all()
    _multi(pkg, [new[:1]], [old[:1] + 1.0], 1.0, (0, 0, 0), "the call after")


def test_multi_layout_64_bits_with_object_bit(pkg, gpu):
    """21 + 21 + 21 bits and two objects: the object bit is bit 63"""
    hi = [(1 << 20) + 5, (1 << 20) + 3, (1 << 20) + 7]
    news = [_cell_points([[0, 0, 0], hi]), _cell_points([[-3, -3, -3], hi, [9, 9, 9]])]
    olds = [_cell_points([hi, [1, 2, 3]]), _cell_points([[9, 9, 9], [0, 0, 0]])]
    ra, rr = _multi(pkg, news, olds, 1.0, (0, 0, 0), "21 + 21 + 21 bits, two objects")
    assert ra.tolist() == [[0, 0, 0, 0], [1, -3, -3, -3], [1] + hi] and rr.tolist() == [[0, 1, 2, 3], [1, 0, 0, 0]]


def test_multi_layout_65_bits_refused(pkg, gpu):
    new = _cell_points([[0, 0, 0], [(1 << 21) + 5, (1 << 20) + 3, (1 << 20) + 7], [-100, 17, -3]])
    with pytest.raises(RuntimeError, match="lattice extent too large for 64-bit keys"):
        pkg.change_detection.voxel_key_diff_multi([new, new[:1]], [new[:1], new], 1.0, (0, 0, 0))
    _multi(pkg, [new[:1], new[:1]], [E3, new[:1] + 2.0], 1.0, (0, 0, 0), "the call after")


# --------------------------------------------------------------------------------------------------- field widths
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_diff_axis_of_extent_zero(pkg, gpu, axis):
    rng = np.random.default_rng(43 + axis)
    new, old = rng.uniform(-2.0, 2.0, (1500, 3)), rng.uniform(-2.0, 2.0, (1500, 3))
    new[:, axis] = rng.uniform(-0.049, -0.001, 1500)  # one cell, index -1
    old[:, axis] = rng.uniform(-0.049, -0.001, 1500)
    ra, rr = _single(pkg, new, old, 0.05, (0, 0, 0), "flat")
    assert (ra[:, axis] == -1).all() and len(ra) > 0 and len(rr) > 0
    _multi(pkg, _split(rng, new, 2), _split(rng, old, 2), 0.05, (0, 0, 0), "flat, 2 objects")


@pytest.mark.parametrize("extent", [1, 2, 255, 256, 511, 512])
def test_diff_extents_at_field_width_steps(pkg, gpu, extent):
    """joint extents of exactly 2^b - 1 cells (b bits) and 2^b cells (b + 1 bits), b = 1, 8, 9, on x; the same extent
    hanging below zero on y; a third of it on z, reached only by the OLD cloud (the bounds are joint)"""
    rng = np.random.default_rng(50 + extent)
    n = 1200

    def draw(zmax, mod, rem):
        c = np.stack([rng.integers(0, extent + 1, n), -rng.integers(0, extent + 1, n), rng.integers(0, zmax + 1, n)], 1)
        c = c[(c[:, 0] + c[:, 1]) % mod != rem]  # the two clouds leave out different cells
        c[0] = [0, -extent, 0]
        c[1] = [extent, 0, zmax]
        return c.astype(np.float64) * 0.25 + rng.uniform(0.01, 0.24, c.shape)

    new, old = draw(0, 2, 0), draw(extent // 3, 3, 1)
    joint = V.cells(np.concatenate([new, old]), 0.25, (0, 0, 0))
    assert (joint.max(0) - joint.min(0)).tolist() == [extent, extent, extent // 3]
    ra, rr = _single(pkg, new, old, 0.25, (0, 0, 0), f"extent {extent}")
    assert len(ra) + len(rr) > 0
    _multi(pkg, _split(rng, new, 3), _split(rng, old, 3), 0.25, (0, 0, 0), f"extent {extent}, 3 objects")


@pytest.mark.parametrize("n_objects", [1, 2, 3, 4, 5, 2048])
def test_multi_object_counts(pkg, gpu, n_objects):
    """bits_for(n_objects - 1) steps at 2, 3 and 5 objects; 2048 is the most the library takes (most objects empty, a
    few points in the first and the last)"""
    rng = np.random.default_rng(60 + n_objects)
    news, olds = [E3] * n_objects, [E3] * n_objects
    for j in sorted({0, n_objects // 2, n_objects - 1}):
        p = rng.uniform(-0.5, 0.5, (300, 3))
        news[j] = p
        olds[j] = np.concatenate([p[:200], rng.uniform(-0.5, 0.5, (100, 3))])
    ra, rr = _multi(pkg, news, olds, 0.04, (0.0, 0.1, -0.1), f"{n_objects} objects")
    assert ra[:, 0].max() == n_objects - 1 and rr[:, 0].max() == n_objects - 1 and ra[:, 0].min() == 0


def test_multi_2049_objects_refused(pkg, gpu):
    p = np.array([[0.1, 0.2, 0.3]])
    with pytest.raises(RuntimeError, match="invalid arguments"):
        pkg.change_detection.voxel_key_diff_multi([p] + [E3] * 2048, [E3] * 2049, 0.04, (0, 0, 0))
    _multi(pkg, [p, E3], [E3, p], 0.04, (0, 0, 0), "the call after")


# ------------------------------------------------------------------------------------------------------ set logic
def test_diff_set_logic(pkg, gpu):
    rng = np.random.default_rng(70)
    origin = (0.3, 0.3, 0.3)
    base = rng.uniform(-1.0, 1.0, (1500, 3))
    dup = np.concatenate([base, base[:700], base[100:400]])
    perm = dup[rng.permutation(len(dup))]
    ra, rr = _single(pkg, dup, perm, 0.05, origin, "same set, permuted with duplicates")
    assert len(ra) == 0 and len(rr) == 0
    ma, mr = _multi(pkg, [dup, base[:9]], [perm, base[:9][::-1]], 0.05, origin, "same sets, 2 objects")
    assert len(ma) == 0 and len(mr) == 0
    left, right = base[base[:, 0] < -0.1], base[base[:, 0] > 0.1]
    ra, rr = _single(pkg, left, right, 0.05, origin, "disjoint")
    assert len(ra) == len(np.unique(V.cells(left, 0.05, origin), axis=0))
    _multi(pkg, [left, right], [right, left], 0.05, origin, "disjoint, swapped in the second object")
    for new, old, what in ((E3, base, "new empty"), (base, E3, "old empty"), (E3, E3, "both empty")):
        _single(pkg, new, old, 0.05, origin, what)
        _multi(pkg, [new, new], [old, old], 0.05, origin, what + ", 2 objects")
    ma, mr = _multi(pkg, [base, E3, left], [base, right, left], 0.05, origin, "an object only in the old map")
    assert len(ma) == 0 and (mr[:, 0] == 1).all() and len(mr) > 0


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_diff_sizes_around_the_sort_tile(pkg, gpu, n):
    rng = np.random.default_rng(80 + n)
    new = rng.uniform(-3.0, 3.0, (n, 3))
    old = np.concatenate([new[: n // 2], rng.uniform(-3.0, 3.0, (n - n // 2, 3))])
    ra, rr = _single(pkg, new, old, 0.05, (0.01, 0.02, 0.03), f"{n} points")
    assert len(ra) > 0
    ma, mr = _multi(pkg, [new, old], [old, new], 0.05, (0.01, 0.02, 0.03), f"{n} points, 2 objects")
    assert len(ma) == len(ra) + len(rr)


# ------------------------------------------------------------------------------------------------ range refusals
OUT_OF_RANGE = "lattice key out of range"


def test_single_range_refusal(pkg, gpu):
    """cells up to +-(2^20 - 1) are keys; 2^20 cells out is refused; so are NaN and inf; each refusal is followed by a
    valid call"""
    cd = pkg.change_detection
    lim = float(1 << 20)
    ok = np.array([[lim - 0.5, 0.5, 0.5], [0.5, -(lim - 1.5), 0.5], [0.5, 0.5, lim - 0.5]])
    ra, rr = _single(pkg, ok, ok[:1] * [1, 1, -1], 1.0, (0, 0, 0), "largest single-form cells")
    assert ra.max() == (1 << 20) - 1 and ra.min() == -((1 << 20) - 1)
    good = np.random.default_rng(90).uniform(-1, 1, (500, 3))
    for bad in (lim + 0.5, -(lim + 1.5), np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = good.copy()
            p[123, axis] = bad
            with pytest.raises(RuntimeError, match=OUT_OF_RANGE):
                cd.voxel_key_diff(p, good, 1.0, (0, 0, 0))
            with pytest.raises(RuntimeError, match=OUT_OF_RANGE):
                cd.voxel_key_diff(good, p, 1.0, (0, 0, 0))
        _single(pkg, good, good[::-1] + 0.3, 0.1, (0, 0, 0), f"the call after refusing {bad}")


def test_multi_range_refusal(pkg, gpu):
    """|cell| < 2^30 in the multi form"""
    cd = pkg.change_detection
    lim = float(1 << 30)
    ok = np.array([[lim - 0.5, 0.5, 0.5], [-(lim - 1.5), 0.5, 0.5]])
    ra, rr = _multi(pkg, [ok, ok[:1]], [E3, ok[1:]], 1.0, (0, 0, 0), "largest multi-form cells")
    assert ra[:, 1].max() == (1 << 30) - 1 and ra[:, 1].min() == -((1 << 30) - 1)
    good = np.random.default_rng(91).uniform(-1, 1, (500, 3))
    for bad in (lim + 0.5, -(lim + 1.5), np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = good.copy()
            p[321, axis] = bad
            with pytest.raises(RuntimeError, match=OUT_OF_RANGE):
                cd.voxel_key_diff_multi([good, p], [good, good], 1.0, (0, 0, 0))
            with pytest.raises(RuntimeError, match=OUT_OF_RANGE):
                cd.voxel_key_diff_multi([good, E3], [p, good], 1.0, (0, 0, 0))
        _multi(pkg, [good, good[:7]], [good[::-1] + 0.3, E3], 0.1, (0, 0, 0), f"the call after refusing {bad}")
