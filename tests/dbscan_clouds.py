"""The designed clouds of the DBSCAN tests (test_dbscan_api.py checks their properties on the CPU and that the
reference's loop and closed form agree on them; test_gpu_dbscan.py runs them on the GPU).  Every cloud has at most
5 000 points.  Each builder returns (points float64 [n][3], eps, min_points) or a list of such cases."""
import numpy as np

import ror_ref as R

EPS_SWEEP = (0.05, 0.08, 0.12, 0.2)
MINPTS_SWEEP = (1, 2, 3, 5, 10)


def blob_cloud(seed, n=None):
    """Gaussian blobs of several widths in the unit cube plus uniform noise, <= 500 points, shuffled"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(150, 501)) if n is None else n
    n_noise = n // 5
    k = int(rng.integers(2, 6))
    centres = rng.uniform(0.1, 0.9, (k, 3))
    which = rng.integers(0, k, n - n_noise)
    sigma = rng.uniform(0.02, 0.08, k)[which]
    pts = np.concatenate([centres[which] + rng.normal(0, 1, (n - n_noise, 3)) * sigma[:, None],
                          rng.uniform(-0.1, 1.1, (n_noise, 3))])
    return pts[rng.permutation(n)]


def random_cases(n_seeds=3):
    """(points, eps, min_points) over the parameter sweep, a different cloud for every case"""
    out = []
    for s in range(n_seeds):
        for a, eps in enumerate(EPS_SWEEP):
            for b, mp in enumerate(MINPTS_SWEEP):
                out.append((blob_cloud(1000 * s + 10 * a + b), eps, mp))
    return out


def _clump(centre, m, eps):
    """m points within 0.02 eps of centre (a short run along z)"""
    c = np.repeat(np.asarray(centre, np.float64)[None], m, 0)
    c[:, 2] += np.arange(m) * (0.02 * eps / max(m, 1))
    return c


CONTESTED_EPS, CONTESTED_MINPTS, CONTESTED_CLUMP, CONTESTED_BORDER = 0.1, 13, 5, 8


def contested():
    """Two parallel rows of clumps (5 points each, clumps 0.9 eps apart, so a clump's points count 15 neighbours: core
    for min_points = 13) 1.5 eps apart in y: row A (y = 0) stored first, row B (y = 1.5 eps) after it.  Between them,
    at y = 0.8 eps (0.8 eps from A, 0.7 eps from B) and level with every fourth clump, single points that see one clump
    of each row: 11 neighbours, not core, core neighbours in both clusters, the nearest of them in B.  The singles
    are stored first, in the middle and last."""
    eps, m = CONTESTED_EPS, CONTESTED_CLUMP
    nclumps = 40
    xs = np.arange(nclumps) * (0.9 * eps)
    row_a = np.concatenate([_clump([x, 0.0, 0.0], m, eps) for x in xs])
    row_b = np.concatenate([_clump([x, 1.5 * eps, 0.0], m, eps) for x in xs])
    singles = np.array([[xs[4 * t + 1], 0.8 * eps, 0.0] for t in range(CONTESTED_BORDER)])
    pts = np.concatenate([singles[:3], row_a, singles[3:6], row_b, singles[6:]])
    single_idx = np.concatenate([np.arange(3), 3 + len(row_a) + np.arange(3),
                                 6 + len(row_a) + len(row_b) + np.arange(CONTESTED_BORDER - 6)])
    return pts, eps, CONTESTED_MINPTS, single_idx


NOISE_FIRST_EPS, NOISE_FIRST_MINPTS = 0.05, 9


def noise_first():
    """Six clusters 10 eps apart: a clump of 6 points with 4 fringe points 0.9 eps from it (at +-x, +-y: more than eps
    from each other).  A clump point counts 10 neighbours (core for min_points = 9), a fringe point 7 (not core).
    All fringe points are stored before every clump, so the loop first marks them noise and the cluster claims them
    afterwards.  Then 20 truly isolated points (3 eps apart on a line 10 eps away)."""
    eps = NOISE_FIRST_EPS
    fringe, clumps = [], []
    for c in range(6):
        centre = np.array([10.0 * eps * c, -3.0, 1.0])
        clumps.append(_clump(centre, 6, eps))
        for d in ([0.9, 0, 0], [-0.9, 0, 0], [0, 0.9, 0], [0, -0.9, 0]):
            fringe.append(centre + np.array(d) * eps + [0, 0, 0.01 * eps])
    lone = np.stack([np.arange(20) * 3.0 * eps, np.full(20, -3.0 + 10 * eps), np.full(20, 1.0)], 1)
    fringe = np.array(fringe)
    pts = np.concatenate([fringe, np.concatenate(clumps), lone])
    return pts, eps, NOISE_FIRST_MINPTS, len(fringe), len(lone)


LATTICE_EPS = 2.0 ** -4


def lattice():
    """6 x 5 x 4 integer lattice (unscaled)"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1)
    return g.reshape(-1, 3).astype(np.float64)


def lattice_cases():
    """(name, points, eps, min_points): the lattice scaled by eps = 2^-4 at exactly eps and one double above it, and
    the lattice scaled by nextafter(eps, 0) with radius eps"""
    e = LATTICE_EPS
    up = float(np.nextafter(e, 1.0))
    pts = lattice() * e
    out = [("at eps", pts, e, 1), ("at eps", pts, e, 2)]
    out += [("above eps", pts, up, mp) for mp in (4, 5, 7, 8)]
    below = lattice() * float(np.nextafter(e, 0.0))
    out += [("scaled below eps", below, e, mp) for mp in (1, 2, 4, 5, 7, 8)]
    return out


def straddle_cases(axis):
    """(points, r, number of miss pairs) per (origin, radius) of ror_ref.straddle_pairs(1.0) with any miss pair: the
    anchor, then up to 400 miss pairs, then up to 200 near pairs, laid along `axis` (min_points = 2)"""
    out = []
    for o, r, miss, near in R.straddle_pairs(1.0):
        if len(miss) == 0 and len(near) == 0:
            continue
        pairs = np.concatenate([miss[:400], near[:200]])
        out.append((R.pair_cloud(o, r, pairs, axis), r, min(len(miss), 400)))
    return out


CHAIN_EPS = 0.03


def chain(n, eps=CHAIN_EPS):
    """n points along a folded line at spacing 0.9 eps: 64 steps along +x, 3 steps along +y, 64 steps along -x, 3 steps
    along +y, ... (rows 2.7 eps apart, so only consecutive points are neighbours)"""
    step = 0.9 * eps
    ij = np.zeros((n, 2), np.int64)
    x = y = 0
    d = 1
    run = 0
    for t in range(1, n):
        if run < 64:
            x += d
            run += 1
        else:
            y += 1
            run += 1
            if run == 67:
                run = 0
                d = -d
        ij[t] = (x, y)
    pts = np.zeros((n, 3))
    pts[:, :2] = ij * step
    return pts + [-1.0, 2.0, 0.5]


def two_chains(n_each=2048, eps=CHAIN_EPS):
    """two chains 5 eps apart in z, interleaved in index order: even indices chain A, odd indices chain B"""
    a = chain(n_each, eps)
    b = a + [0.0, 0.0, 5.0 * eps]
    pts = np.empty((2 * n_each, 3))
    pts[0::2] = a
    pts[1::2] = b
    return pts


COINCIDENT_EPS, COINCIDENT_M = 0.05, 5


def coincident():
    """Groups of m - 1, m and m + 1 identical points (min_points = m) at the origin, at negative coordinates and at
    +-10^3, 10 apart, shuffled.  Returns (points, eps, m, group size of every point, group id of every point)."""
    m = COINCIDENT_M
    rng = np.random.default_rng(41)
    places = np.array([[0.0, 0.0, 0.0], [-1000.0, 3.0, 7.0], [1000.0, -1000.0, 0.5], [12.3, 1000.0, -1000.0],
                       [-0.37, -2.5, -1.25]])
    parts, sizes, gid = [], [], []
    for a, base in enumerate(places):
        for b, k in enumerate((m - 1, m, m + 1)):
            parts.append(np.repeat((base + [10.0 * b, 0.0, 0.0])[None], k, 0))
            sizes += [k] * k
            gid += [3 * a + b] * k
    perm = rng.permutation(len(sizes))
    return np.concatenate(parts)[perm], COINCIDENT_EPS, m, np.array(sizes)[perm], np.array(gid)[perm]


def small_cases():
    """(name, points, eps, min_points): n = 1, 2, 256, 257, min_points > n, min_points = 0"""
    rng = np.random.default_rng(43)
    one = np.array([[0.3, -0.2, 5.0]])
    two = np.array([[0.3, -0.2, 5.0], [0.3, -0.25, 5.0]])
    out = []
    for mp in (0, 1, 2):
        out.append(("n = 1", one, 0.1, mp))
    for mp in (0, 1, 2, 3):
        out.append(("n = 2, neighbours", two, 0.1, mp))
        out.append(("n = 2, apart", two, 0.04, mp))
    for n in (256, 257):
        pts = rng.normal(0, 0.05, (n, 3))
        for mp in (0, 4, n + 1):
            out.append((f"n = {n}", pts, 0.03, mp))
    blob = rng.uniform(-0.01, 0.01, (50, 3)) - 3.0  # every point within eps of every other
    for mp in (50, 51, 1000):
        out.append(("blob of 50", blob, 0.1, mp))
    return out
