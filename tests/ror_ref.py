"""numpy restatement of PointCloud::RemoveRadiusOutliers (the checker of test_filter_refs.py and
test_gpu_ror_edges.py), and the search for point pairs that straddle the cells of a radius-sized neighbour grid.

Exhaustive and float64: count_i = |{j : ((dx dx) + dy dy) + dz dz < r r}| over ALL j (point i itself included, as the
radius search returns the query), point i is kept iff count_i > nb_points.  The association is nanoflann's L2 order,
the one d2_l2 (csrc/grid.h) and the oracle's dist2 use; numpy evaluates every product and sum as its own rounded
float64 operation, so the comparison sees the same bits.  No search structure: nothing here knows about cells.
"""
import functools

import numpy as np


def neighbour_counts(xyz, radius, chunk=256):
    """count_i of every point (int64 [n]), self included"""
    P = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
    n = P.shape[0]
    r2 = np.float64(radius) * np.float64(radius)
    cnt = np.zeros(n, np.int64)
    for s in range(0, n, chunk):
        q = P[s:s + chunk]
        dx = q[:, None, 0] - P[None, :, 0]
        dy = q[:, None, 1] - P[None, :, 1]
        dz = q[:, None, 2] - P[None, :, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        cnt[s:s + chunk] = (d2 < r2).sum(1)
    return cnt


def remove_radius_outlier(xyz, nb_points, radius):
    """kept indices (int64, ascending)"""
    if nb_points < 1 or not radius > 0:
        raise RuntimeError("Illegal input parameters")
    return np.nonzero(neighbour_counts(xyz, radius) > nb_points)[0].astype(np.int64)


# ------------------------------------------------------------------------------------------------ cell straddles
def cell_of(v, o, h):
    """the cell a radius-sized grid anchored at o gives coordinate v: floor((v - o) / h), each operation rounded"""
    return np.floor((np.asarray(v, np.float64) - np.float64(o)) / np.float64(h))


def step_ulps(v, k):
    """v moved by k representable doubles (k may be negative); v finite and well inside a binade range"""
    v = np.asarray(v, np.float64)
    bits = v.view(np.int64) if v.ndim else np.array([v]).view(np.int64)
    # positive doubles order as their bit patterns, negative ones in reverse
    moved = np.where(bits >= 0, bits + k, bits - k)
    return moved.view(np.float64).reshape(v.shape)


def straddle_search(o, r, k_lo, k_hi, width=6, h=None):
    """Pairs (v2, v1), v2 < v1, among the doubles within `width` steps of the faces o + k h of a grid of cell size h
    (default: h = r) anchored at o, k_lo <= k < k_hi: v2 next to face k, v1 next to (face k) + r.  Returns
    (miss, near):

    * miss: pairs with (v1 - v2)^2 < r r whose cells differ by 2 or more -- neighbours that a scan of the 3x3x3 block
      of the grid never meets;
    * near: pairs whose cells differ by exactly 1 and whose separation is within 4 doubles of r, on either side of it
      (both outcomes of the strict <).
    """
    o, r = np.float64(o), np.float64(r)
    h = r if h is None else np.float64(h)
    k = np.arange(k_lo, k_hi, dtype=np.float64)
    steps = np.arange(-width, width + 1)
    face = o + k * h
    lo = np.stack([step_ulps(face, int(s)) for s in steps], 1)      # [K][W] next to face k
    hi = np.stack([step_ulps(face + r, int(s)) for s in steps], 1)  # [K][W] one radius on
    v2 = lo[:, :, None]
    v1 = hi[:, None, :]
    d = v1 - v2
    inside = (d * d) < r * r
    dc = cell_of(v1, o, h) - cell_of(v2, o, h)
    miss = inside & (dc >= 2)
    r_lo, r_hi = step_ulps(r, -4), step_ulps(r, 4)
    near = (dc == 1) & (d >= r_lo) & (d <= r_hi)

    def pairs(mask, per_face):
        out = []
        for i in np.nonzero(mask.any(axis=(1, 2)))[0]:
            a, b = np.nonzero(mask[i])
            for t in range(min(per_face, a.size)):
                out.append((lo[i, a[t]], hi[i, b[t]]))
        return np.array(out, np.float64).reshape(-1, 2)

    return pairs(miss, 1), pairs(near, 1)


# the (origin / r, r) configurations the straddle tests cover: non-dyadic radii and a dyadic one, the cloud minimum at
# zero, a few radii below zero, and 517 to 3000 radii either side of it (the points lie 100 .. 10 000 radii above the
# minimum, i.e. at coordinates of -2900 .. +10 500 radii)
STRADDLE_RADII = (0.1, 0.02, 0.016, 2.0 ** -4)
STRADDLE_ORIGINS = (0.0, -73.0, -1000.123, -3000.7, 517.77)  # in units of r
STRADDLE_FACES = (100, 10000)
ROR_CELL_SCALE = 1.0 + 2.0 ** -20  # csrc/grid.h


@functools.lru_cache(maxsize=None)
def straddle_pairs(h_scale=1.0):
    """[(o, r, miss pairs, near pairs)] over STRADDLE_RADII x STRADDLE_ORIGINS for a grid of cell size r * h_scale"""
    out = []
    for r in STRADDLE_RADII:
        for ou in STRADDLE_ORIGINS:
            o = ou * r
            miss, near = straddle_search(o, r, *STRADDLE_FACES, h=r * h_scale)
            out.append((o, r, miss, near))
    return out


def pair_cloud(o, r, pairs, axis, max_pairs=1200):
    """The pairs laid along `axis`, each on its own row 4 r from the next along the following axis (so a point's only
    candidate neighbour is its partner), plus one anchor point at coordinate o that makes o the cloud's minimum."""
    pairs = pairs[:max_pairs]
    m = pairs.shape[0]
    pts = np.zeros((2 * m + 1, 3))
    row = np.arange(m, dtype=np.float64) * (4.0 * r)
    b = (axis + 1) % 3
    pts[0, axis] = o
    pts[1::2, axis] = pairs[:, 0]
    pts[2::2, axis] = pairs[:, 1]
    pts[1::2, b] = row
    pts[2::2, b] = row
    return pts
