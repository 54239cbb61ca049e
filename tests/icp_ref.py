"""numpy restatement of the registration definition in DESIGN.md §4 (the checker of test_registration_api.py and
test_gpu_registration.py), and the analytic test scene.

Nearest neighbours are exhaustive (chunked), d2 = ((dx dx) + dy dy) + dz dz, equidistant targets go to the lowest
index (np.argmin returns the first minimum), a correspondence needs d2 < r r, the transform is Eigen's column-order
product, the fit is umeyama without scaling on np.linalg.svd.
"""
import functools

import numpy as np

R_CORR = 0.05


def transform_points(P, T):
    P = np.asarray(P, np.float64)
    v = [((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3] for r in range(4)]
    return np.stack([v[0] / v[3], v[1] / v[3], v[2] / v[3]], axis=1)


def transform_normals(N, T):
    N = np.asarray(N, np.float64)
    return np.stack([(T[r, 0] * N[:, 0] + T[r, 1] * N[:, 1]) + T[r, 2] * N[:, 2] for r in range(3)], axis=1)


def rotate_matrix(R, c):
    """the rigid transform PointCloud.rotate(R, center=c) runs: [R | c - R c]"""
    T = np.eye(4)
    T[:3, :3] = R
    for i in range(3):
        T[i, 3] = c[i] - ((R[i, 0] * c[0] + R[i, 1] * c[1]) + R[i, 2] * c[2])
    return T


def rotation_xyz_closed_form(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.array([[cb * cc, -cb * sc, sb],
                     [ca * sc + sa * sb * cc, ca * cc - sa * sb * sc, -sa * cb],
                     [sa * sc - ca * sb * cc, sa * cc + ca * sb * sc, ca * cb]])


def nearest(P, Q, chunk=512):
    """per row of P: (d2, index) of its nearest row of Q and the second-smallest d2 (inf for a one-point Q)"""
    n = P.shape[0]
    d2 = np.empty(n)
    idx = np.empty(n, np.int64)
    second = np.full(n, np.inf)
    for s in range(0, n, chunk):
        p = P[s:s + chunk]
        dx = p[:, None, 0] - Q[None, :, 0]
        dy = p[:, None, 1] - Q[None, :, 1]
        dz = p[:, None, 2] - Q[None, :, 2]
        D = ((dx * dx) + dy * dy) + dz * dz
        j = np.argmin(D, axis=1)
        rows = np.arange(p.shape[0])
        d2[s:s + chunk] = D[rows, j]
        idx[s:s + chunk] = j
        if Q.shape[0] > 1:
            D[rows, j] = np.inf
            second[s:s + chunk] = D.min(axis=1)
    return d2, idx, second


class Result:
    pass


def evaluate(P, Q, r):
    """evaluate_registration of an already transformed cloud P against Q"""
    res = Result()
    n = P.shape[0]
    if n == 0 or Q.shape[0] == 0:
        res.d2, res.idx = np.zeros(n), np.full(n, -1, np.int64)
        res.second = np.full(n, np.inf)
        res.corr = np.zeros((0, 2), np.int32)
        res.fitness = res.inlier_rmse = 0.0
        return res
    d2, idx, second = nearest(P, Q)
    ok = d2 < r * r
    k = int(ok.sum())
    res.d2, res.idx, res.second = d2, np.where(ok, idx, -1), second
    res.corr = np.stack([np.nonzero(ok)[0], idx[ok]], axis=1).astype(np.int32)
    res.fitness = k / n if k else 0.0
    res.inlier_rmse = float(np.sqrt(d2[ok].sum() / k)) if k else 0.0
    return res


def fit(P, Q, corr):
    """Eigen::umeyama(P[corr[:, 0]] -> Q[corr[:, 1]]) without scaling"""
    if corr.shape[0] == 0:
        return np.eye(4)
    p, q = P[corr[:, 0]], Q[corr[:, 1]]
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    S = (q - mq).T @ (p - mp) / p.shape[0]
    U, _, Vt = np.linalg.svd(S)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ np.diag(d) @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp(src, tgt, r, init, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """registration_icp; the result also carries the trajectory's smallest best/second-best gap and smallest relative
    distance of a d2 from r r (the preconditions of the parity tests), over every evaluation"""
    assert r > 0
    T = np.array(init, np.float64)
    pcd = np.asarray(src, np.float64)
    if not np.array_equal(T, np.eye(4)):
        pcd = transform_points(pcd, T)
    res = evaluate(pcd, tgt, r)
    gap, margin = [], []

    def note(e):
        if e.d2.size and tgt.shape[0]:
            gap.append(float(np.min(e.second - e.d2)))
            margin.append(float(np.min(np.abs(e.d2 - r * r) / (r * r))))

    note(res)
    iterations = 0
    for _ in range(max_iteration):
        up = fit(pcd, tgt, res.corr)
        T = up @ T
        pcd = transform_points(pcd, up)
        backup, res = res, evaluate(pcd, tgt, r)
        note(res)
        iterations += 1
        if abs(backup.fitness - res.fitness) < relative_fitness and \
                abs(backup.inlier_rmse - res.inlier_rmse) < relative_rmse:
            break
    res.transformation, res.iterations = T, iterations
    res.min_gap = min(gap) if gap else np.inf
    res.min_margin = min(margin) if margin else np.inf
    return res


# ------------------------------------------------------------------------------------------------ the test scene
def _axis_rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


@functools.lru_cache(maxsize=None)
def scene(deg):
    """(source [2800, 3], target [4800, 3], T_gt): three 40x40 jittered 4 cm lattices (a bumpy floor, two wavy walls)
    placed where the evaluation maps sit; the source is 2500 target points moved by inverse(T_gt) -- a rotation of
    `deg` degrees about (0.3, -0.5, 0.8) through the centroid plus a 1.8 cm translation -- and 300 of them shifted
    by +0.5 m per axis (no correspondence: beyond r, many outside the target's box)."""
    rng = np.random.default_rng(20240 + int(deg))
    g = np.arange(40) * 0.04
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    ju, jv = rng.uniform(-0.014, 0.014, (2, 3, u.size))
    floor = np.stack([u + ju[0], v + jv[0], 0.015 * np.sin(5.0 * u) * np.cos(3.7 * v)], axis=1)
    wall_x = np.stack([0.02 * np.sin(4.1 * v + 2.3 * u) - 0.03, u + ju[1], v + jv[1] + 0.03], axis=1)
    wall_y = np.stack([u + ju[2], 0.02 * np.cos(3.3 * u - 2.9 * v) - 0.03, v + jv[2] + 0.03], axis=1)
    tgt = np.concatenate([floor, wall_x, wall_y]) + np.array([-4.5, 5.6, 0.3])
    c = tgt.mean(axis=0)
    T_gt = np.eye(4)
    T_gt[:3, :3] = _axis_rotation((0.3, -0.5, 0.8), deg)
    T_gt[:3, 3] = c - T_gt[:3, :3] @ c + np.array([0.010, -0.012, 0.009])
    pick = rng.permutation(tgt.shape[0])[:2500]
    src = transform_points(tgt[pick], np.linalg.inv(T_gt))
    far = src[rng.permutation(2500)[:300]] + 0.5
    return np.ascontiguousarray(np.concatenate([src, far])), np.ascontiguousarray(tgt), T_gt


@functools.lru_cache(maxsize=None)
def reference_icp(deg, max_iteration=30):
    src, tgt, _ = scene(deg)
    return icp(src, tgt, R_CORR, np.eye(4), max_iteration=max_iteration)
