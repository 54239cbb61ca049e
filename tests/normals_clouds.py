"""The designed clouds of test_normals_api.py (CPU: their properties) and test_gpu_normals.py (GPU parity), each at
most 5 000 points, and their references (tests/normals_ref.py), computed once per process and never modified.

A case is (points, k, radius or None, prior normals or None); radius None is KDTreeSearchParamKNN(k), otherwise
KDTreeSearchParamHybrid(radius, k)."""
import functools

import numpy as np

import normals_ref as NR
import ror_ref as R

OFFSET = np.array([1.0, -2.0, 0.5])
LATTICE_H = 2.0 ** -6


def box_cloud(seed=7, n=1500, noise=0.001):
    """a floor patch and two box faces meeting it, 1 mm noise, away from the origin"""
    rng = np.random.default_rng(seed)
    m = n // 3
    u = rng.uniform(-0.25, 0.25, (n, 2))
    parts = [np.c_[u[:m], np.zeros(m)],
             np.c_[u[m:2 * m, 0], np.full(m, 0.25), u[m:2 * m, 1] + 0.25],
             np.c_[np.full(n - 2 * m, -0.25), u[2 * m:, 0], u[2 * m:, 1] + 0.25]]
    return np.vstack(parts) + rng.normal(0, noise, (n, 3)) + OFFSET


def lattice():
    """12 x 12 points of the plane z = 0.25 at spacing 2^-6: every sum of the covariance is exact"""
    g = np.arange(12, dtype=np.float64) * LATTICE_H
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.c_[x.ravel() + 1.0, y.ravel() - 2.0, np.full(144, 0.25)]


def coincident(k=8):
    """groups of k + 4 coincident points (more than k: a point's neighbours are the k lowest indices of its group),
    stored interleaved; dyadic coordinates make every sum exact, so the covariance is the zero matrix; one more group
    at coordinates that are not dyadic"""
    sites = np.array([[0.5, 1.25, -0.75], [0.5, 1.25, 3.0], [-2.0, 0.125, 1.0], [0.3, -0.7, 1.1]])
    gid = np.tile(np.arange(len(sites)), k + 4)
    return sites[gid], gid


def line(n=40):
    t = np.arange(n, dtype=np.float64)[:, None] * 0.0137
    return t * np.array([1.0, 2.0, 3.0]) + OFFSET


def far_point():
    """a dense 0.1 x 0.1 patch and one point 3 units away: dozens of cells of any grid sized for the patch"""
    rng = np.random.default_rng(11)
    patch = np.c_[rng.uniform(0, 0.1, (500, 2)), rng.normal(0, 0.0005, 500)]
    return np.vstack([patch, [[3.0, 0.02, 0.01]]]) + OFFSET


def straddle_cloud(axis):
    """cell-straddling and near-radius pairs of ror_ref.straddle_pairs laid along `axis`; returns (points, r)"""
    for o, r, miss, near in R.straddle_pairs(1.0):
        if len(miss) and len(near):
            pairs = np.concatenate([miss[:200], near[:100]])
            return R.pair_cloud(o, r, pairs, axis), r
    raise AssertionError("no straddling configuration")


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = np.c_[rng.uniform(-0.2, 0.2, (n, 2)), rng.normal(0, 0.002, n)]
    return p + OFFSET


def priors(n, seed, zeros=(0, 5, 17)):
    """unit prior normals in random directions, some of them zero"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    for z in zeros:
        if z < n:
            v[z] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, k, radius, prior)"""
    c = {}
    for n in (1, 2, 3, 29, 30, 31):
        c[f"n{n}_k30"] = (random_cloud(n, 100 + n), 30, None, None)
    for n in (63, 64, 65):
        c[f"n{n}_k64"] = (random_cloud(n, 200 + n), 64, None, None)
    for n in (63, 64, 65, 255, 256, 257):
        c[f"n{n}_k30"] = (random_cloud(n, 300 + n), 30, None, None)
    p257 = random_cloud(257, 557)
    for k in (1, 2, 3, 32, 33, 64):
        c[f"n257_k{k}"] = (p257, k, None, None)
    c["n257_hybrid_k64"] = (p257, 64, 0.05, None)
    box = box_cloud()
    c["box_k30"] = (box, 30, None, None)
    c["box_k10"] = (box, 10, None, None)
    c["box_hybrid"] = (box, 30, 0.03, None)   # the radius binds: 1 .. 17 neighbours
    c["box_hybrid_k5"] = (box, 5, 0.03, None)  # max_nn binds for most points, the radius for the rest
    c["box_permuted"] = (box[np.random.default_rng(8).permutation(len(box))], 30, None, None)
    c["box_priors"] = (box[::3], 30, None, priors(len(box[::3]), 9))
    lat = lattice()
    c["lattice_k16"] = (lat, 16, None, None)
    c["lattice_hybrid_at_spacing"] = (lat, 16, LATTICE_H, None)
    c["lattice_hybrid_above_spacing"] = (lat, 16, float(np.nextafter(LATTICE_H, 1.0)), None)
    co, _ = coincident()
    c["coincident_k8"] = (co, 8, None, None)
    c["coincident_priors"] = (co, 8, None, priors(len(co), 10, zeros=(0, 1, 2, 3)))
    c["line_k10"] = (line(), 10, None, None)
    c["far_point_k30"] = (far_point(), 30, None, None)
    for axis in range(3):
        pts, r = straddle_cloud(axis)
        c[f"straddle_hybrid_axis{axis}"] = (pts, 4, float(r), None)
        c[f"straddle_k3_axis{axis}"] = (pts, 3, None, None)
    return c


# checked by covariance and path code only: their two smallest eigenvalues coincide by design
EXEMPT_FROM_GAP_RULE = ("line_k10", "coincident_k8", "coincident_priors")


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, k, radius, prior = cases()[name]
    assert len(pts) <= 5000
    return NR.estimate(pts, k, radius, prior, longdouble=True)


def tolerance(ref):
    """(compared mask, limit in radians) of a cloud's path-3 normals: points whose reference gap is >= 1e-3; the limit
    is 16 x the largest angle between the float64 reference and its long-double run over them (the reference's own
    rounding sensitivity; 16 covers a few ulp in two library calls), not below 64 * 2^-53"""
    mask = (ref["path"] == NR.PATH_TRIG) & (ref["gap"] >= 1e-3)
    worst = float(NR.angle(ref["normals"][mask], ref["normals_ld"][mask]).max()) if mask.any() else 0.0
    return mask, max(16.0 * worst, 64.0 * 2.0 ** -53), worst
