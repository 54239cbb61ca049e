"""numpy restatement of PointCloud.segment_plane ("Plane segmentation"): Open3D's PointCloud::SegmentPlane
with the seeded counter sampler of this build.  Two statements of the same definition:

  segment_plane_loop : the literal serial loop -- every iteration samples, fits, evaluates fitness and inlier_rmse and
                       compares with the best so far;
  segment_plane      : the closed form the GPU computes -- inlier counts of a chunk of candidates, the loop replayed on
                       the counts alone, inlier_rmse only among the evaluated candidates that hold the best count.

All arithmetic is float64 in the parenthesisation of the definition; serial sums are numpy.cumsum over a leading +0.0
(cumsum adds in index order), never numpy.sum (pairwise).  The break threshold uses math.log / math.pow, the C
library's functions, as the host code does.

Both return a Result: plane (4,), inliers (int64, ascending), evaluated (iterations counted), skipped (zero planes met
before the loop broke), margin (the smallest distance from an integer of any break quotient that trunc() could change,
i.e. finite and below num_iterations + 1; inf if there was none), broke (an iteration was skipped by the break test)
-- these six agree between the two -- and rmse_decided / ties: the equal-fitness comparisons that replaced the best and
all of them (the loop counts them against the best of the moment, the closed form among the final holders only).
"""
import math
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "plane inliers evaluated skipped rmse_decided ties margin broke")

M64 = (1 << 64) - 1
CHUNK = 256  # candidates per batch of the closed form (any value gives the same result)


def rng_word(seed, ctr):
    """splitmix64 of seed + (ctr + 1) * golden: the word csrc/rng.h forms (rng_u01 keeps its top 53 bits)"""
    z = (seed + (ctr + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, it, n, ransac_n):
    """the first ransac_n distinct indices among z(seed, (it << 32) + t) mod n, t = 0, 1, ..., in draw order"""
    kept, t = [], 0
    while len(kept) < ransac_n:
        i = rng_word(seed & M64, ((it << 32) + t) & M64) % n
        if i not in kept:
            kept.append(i)
        t += 1
    return kept


def serial(v):
    """((0 + v0) + v1) + ..."""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(np.concatenate([[0.0], v]))[-1])


def triangle_plane(p0, p1, p2):
    e0 = [float(p1[a]) - float(p0[a]) for a in range(3)]
    e1 = [float(p2[a]) - float(p0[a]) for a in range(3)]
    a = e0[1] * e1[2] - e0[2] * e1[1]
    b = e0[2] * e1[0] - e0[0] * e1[2]
    c = e0[0] * e1[1] - e0[1] * e1[0]
    norm = math.sqrt((a * a + b * b) + c * c)
    if norm == 0.0:
        return np.zeros(4)
    a, b, c = a / norm, b / norm, c / norm
    return np.array([a, b, c, -((a * float(p0[0]) + b * float(p0[1])) + c * float(p0[2]))])


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")  # (NaN compares false: stays NaN)


def plane_from_points(pts, idx):
    """GetPlaneFromPoints over pts[idx] in the order of idx"""
    P = np.ascontiguousarray(pts[np.asarray(idx, np.int64)], np.float64).reshape(-1, 3)
    k = np.float64(len(P))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = [np.float64(serial(P[:, a])) / k for a in range(3)]  # no points: 0 / 0
    r = [P[:, a] - c[a] for a in range(3)]
    xx, xy, xz = serial(r[0] * r[0]), serial(r[0] * r[1]), serial(r[0] * r[2])
    yy, yz, zz = serial(r[1] * r[1]), serial(r[1] * r[2]), serial(r[2] * r[2])
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        a, b, g = det_x, xz * yz - xy * zz, xy * yz - xz * yy
    elif det_y > det_z:
        a, b, g = xz * yz - xy * zz, det_y, xy * xz - yz * xx
    else:
        a, b, g = xy * yz - xz * yy, xy * xz - yz * xx, det_z
    norm = _sqrt((a * a + b * b) + g * g)
    if norm == 0.0:
        return np.zeros(4)
    a, b, g = a / norm, b / norm, g / norm
    return np.array([a, b, g, -((a * float(c[0]) + b * float(c[1])) + g * float(c[2]))])


def candidate(pts, seed, it, ransac_n):
    idx = sample(seed, it, len(pts), ransac_n)
    if ransac_n == 3:
        return triangle_plane(pts[idx[0]], pts[idx[1]], pts[idx[2]])
    return plane_from_points(pts, idx)


def is_zero(plane):
    return bool((plane == 0.0).all())


def distances(pts, plane):
    a, b, c, d = (np.float64(v) for v in plane)
    return np.abs(((a * pts[:, 0] + b * pts[:, 1]) + c * pts[:, 2]) + d)


def break_quotient(fitness, ransac_n, probability):
    """log(1 - probability) / log(1 - fitness^ransac_n) with IEEE division (inf and NaN as they come)"""
    num = math.log(1.0 - probability) if probability < 1.0 else -math.inf
    den_arg = 1.0 - math.pow(fitness, float(ransac_n))
    den = math.log(den_arg) if den_arg > 0.0 else -math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(num) / np.float64(den))


def break_iteration(fitness, ransac_n, probability, num_iterations, margins):
    if not fitness < 1.0:
        return 0
    q = break_quotient(fitness, ransac_n, probability)
    if not (math.isfinite(q) and q >= 0.0):
        return num_iterations
    if q < num_iterations + 1:
        margins.append(min(q - math.floor(q), math.ceil(q) - q) if q != math.floor(q) else 0.0)
    return int(min(math.trunc(q), num_iterations))


def _finish(pts, thr, best_plane, evaluated, skipped, decided, ties, margins, broke):
    if is_zero(best_plane):
        inliers = np.zeros(0, np.int64)
    else:
        inliers = np.nonzero(distances(pts, best_plane) < thr)[0].astype(np.int64)
    return Result(plane_from_points(pts, inliers), inliers, evaluated, skipped, decided, ties,
                  min(margins) if margins else math.inf, broke)


def _check_args(n, ransac_n, probability):
    if not (probability > 0.0 and probability <= 1.0):
        raise RuntimeError("Probability must be > 0 and <= 1.0")
    if ransac_n < 3:
        raise RuntimeError("ransac_n should be set to higher than or equal to 3.")
    if n < ransac_n:
        raise RuntimeError("There must be at least 'ransac_n' points.")


def segment_plane_loop(pts, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0):
    """(a) the literal serial loop"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n, thr = len(pts), float(distance_threshold)
    _check_args(n, ransac_n, probability)
    best_fit, best_rmse, best_plane = 0.0, 0.0, np.zeros(4)
    brk, count = math.inf, 0
    skipped = decided = ties = 0
    margins, broke = [], False
    for it in range(max(num_iterations, 0)):
        if count > brk:
            broke = True
            continue
        plane = candidate(pts, seed, it, ransac_n)
        if is_zero(plane):
            skipped += 1
            continue
        dist = distances(pts, plane)
        inl = dist < thr
        k = int(inl.sum())
        fitness = float(np.float64(k) / np.float64(n))
        rmse = serial(dist[inl]) / math.sqrt(float(k)) if k else 0.0
        if fitness == best_fit and k:
            ties += 1
        if fitness > best_fit or (fitness == best_fit and rmse < best_rmse):
            if fitness == best_fit:
                decided += 1
            best_fit, best_rmse, best_plane = fitness, rmse, plane
            brk = break_iteration(fitness, ransac_n, probability, num_iterations, margins)
        count += 1
    return _finish(pts, thr, best_plane, count, skipped, decided, ties, margins, broke)


def segment_plane(pts, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0):
    """(b) the closed form: counts per chunk, the loop replayed on counts, rmse among the holders of the best count"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n, thr = len(pts), float(distance_threshold)
    _check_args(n, ransac_n, probability)
    x, y, z = (np.ascontiguousarray(pts[:, a]) for a in range(3))
    best_k, holders = 0, []  # holders: planes of the evaluated candidates with count best_k, in iteration order
    brk, count, skipped = math.inf, 0, 0
    margins, broke = [], False
    for it0 in range(0, max(num_iterations, 0), CHUNK):
        if broke:
            break
        its = range(it0, min(it0 + CHUNK, num_iterations))
        planes = np.array([candidate(pts, seed, it, ransac_n) for it in its]).reshape(-1, 4)
        A, B, C, Dd = (planes[:, j][:, None] for j in range(4))
        counts = (np.abs(((A * x + B * y) + C * z) + Dd) < thr).sum(axis=1)
        zero = (planes == 0.0).all(axis=1)
        for c in range(len(planes)):
            if count > brk:
                broke = True
                break
            if zero[c]:
                skipped += 1
                continue
            k = int(counts[c])
            if k > best_k:
                best_k, holders = k, [planes[c]]
                brk = break_iteration(float(np.float64(k) / np.float64(n)), ransac_n, probability, num_iterations,
                                      margins)
            elif k == best_k and k > 0:
                holders.append(planes[c])
            count += 1
    best_plane, decided = np.zeros(4), 0
    if holders:
        best_plane = holders[0]
        if len(holders) > 1:
            root = math.sqrt(float(best_k))
            best_rmse = None
            for h in holders:
                dist = distances(pts, h)
                rmse = serial(np.where(dist < thr, dist, 0.0)) / root  # + 0.0 on a non-negative partial sum is exact
                if best_rmse is None:
                    best_rmse = rmse
                elif rmse < best_rmse:
                    best_rmse, best_plane = rmse, h
                    decided += 1
    return _finish(pts, thr, best_plane, count, skipped, decided, max(len(holders) - 1, 0), margins, broke)
