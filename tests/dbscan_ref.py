"""numpy restatement of PointCloud::ClusterDBSCAN (the checker of test_dbscan_api.py and test_gpu_dbscan.py), twice:
Open3D's literal loop and the closed form the GPU computes (csrc/cluster.hip).

Exhaustive and float64: nbs[i] = {j : ((dx dx) + dy dy) + dz dz < eps eps} over ALL j (point i itself included, as the
radius search returns the query), ascending.  The association is nanoflann's L2 order, the one d2_l2 (csrc/grid.h)
uses; numpy evaluates every product and sum as its own rounded float64 operation, so the comparison sees the same
bits.  No search structure: nothing here knows about cells.
"""
from collections import deque

import numpy as np


def neighbour_lists(xyz, eps, chunk=256):
    """nbs[i] (int64, ascending) of every point, self included"""
    P = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
    n = P.shape[0]
    e2 = np.float64(eps) * np.float64(eps)
    nbs = []
    for s in range(0, n, chunk):
        q = P[s:s + chunk]
        dx = q[:, None, 0] - P[None, :, 0]
        dy = q[:, None, 1] - P[None, :, 1]
        dz = q[:, None, 2] - P[None, :, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        inside = d2 < e2
        nbs += [np.nonzero(row)[0] for row in inside]
    return nbs


def _check_args(eps, min_points):
    if not (eps > 0 and np.isfinite(eps)) or min_points < 0:
        raise RuntimeError("[ClusterDBSCAN] Illegal input parameters")


def loop_labels(nbs, min_points):
    """Open3D's loop over precomputed neighbour lists: labels int32 [n]"""
    n = len(nbs)
    labels = np.full(n, -2, np.int32)
    c = 0
    for i in range(n):
        if labels[i] != -2:
            continue
        if len(nbs[i]) < min_points:
            labels[i] = -1
            continue
        labels[i] = c
        queued = np.zeros(n, bool)  # in the work set now or taken from it before (Open3D: nbs_next + nbs_visited)
        queued[i] = True
        queued[nbs[i]] = True
        work = deque(int(j) for j in nbs[i] if j != i)
        while work:
            nb = work.popleft()
            if labels[nb] == -1:  # noise becomes a border point and is not expanded
                labels[nb] = c
            if labels[nb] != -2:
                continue
            labels[nb] = c
            if len(nbs[nb]) >= min_points:
                for q in nbs[nb]:
                    if not queued[q]:
                        queued[q] = True
                        work.append(int(q))
        c += 1
    return labels


def closed_labels(nbs, min_points):
    """The closed form: core points, their connected components numbered by ascending smallest core index, non-core
    points the smallest label among their core neighbours (-1: none).  Returns (labels int32 [n], core bool [n])."""
    n = len(nbs)
    core = np.array([len(nb) >= min_points for nb in nbs], bool).reshape(n)
    labels = np.full(n, -1, np.int32)
    c = 0
    for i in range(n):
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = c
        stack = [i]
        while stack:
            a = stack.pop()
            for b in nbs[a]:
                if core[b] and labels[b] < 0:
                    labels[b] = c
                    stack.append(int(b))
        c += 1
    for i in np.nonzero(~core)[0]:
        cn = nbs[i][core[nbs[i]]]
        if cn.size:
            labels[i] = labels[cn].min()
    return labels, core


def cluster_dbscan_loop(xyz, eps, min_points):
    _check_args(eps, min_points)
    return loop_labels(neighbour_lists(xyz, eps), min_points)


def cluster_dbscan(xyz, eps, min_points):
    """labels int32 [n] by the closed form"""
    _check_args(eps, min_points)
    return closed_labels(neighbour_lists(xyz, eps), min_points)[0]


def both(xyz, eps, min_points):
    """(loop labels, closed-form labels, core flags, neighbour lists) from one set of neighbour lists"""
    _check_args(eps, min_points)
    nbs = neighbour_lists(xyz, eps)
    closed, core = closed_labels(nbs, min_points)
    return loop_labels(nbs, min_points), closed, core, nbs
