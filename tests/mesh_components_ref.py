"""numpy / plain-Python reference of TriangleMesh.cluster_connected_triangles and the triangle clean-up calls
(csrc/mesh_components.hip, DESIGN.md §4 "mesh components").  No device.

cluster_loop() is Open3D's ClusterConnectedTriangles as written: an edge map, an adjacency list, then tidx ascending
with a breadth-first fill from every unlabelled triangle.  cluster_closed() is the closed form the GPU computes: the
connected components of "shares an edge key (min, max)", numbered by ascending smallest triangle index.  The clean-up
operations are plain sequential loops."""
import math
from collections import deque

import numpy as np


def _tri(triangles):
    return np.ascontiguousarray(np.asarray(triangles, np.int32).reshape(-1, 3))


def edge_keys(triangles):
    """[T][3][2] int64: the (min, max) keys of (a, b), (b, c), (c, a), (a, a) of a degenerate triangle included"""
    t = _tri(triangles).astype(np.int64)
    e = np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=1)
    return np.sort(e, axis=2)


def sorted_edge_positions(triangles):
    """the edge keys in the order of the device's sorted key array (ascending (min, max)): [3T][2], and for every
    distinct key the half-open range of positions it occupies"""
    k = edge_keys(triangles).reshape(-1, 2)
    order = np.lexsort((k[:, 1], k[:, 0]))
    k = k[order]
    runs = {}
    start = 0
    for i in range(1, len(k) + 1):
        if i == len(k) or (k[i] != k[start]).any():
            runs[(int(k[start, 0]), int(k[start, 1]))] = (start, i)
            start = i
    return k, runs


def triangle_areas(vertices, triangles):
    """TriangleMesh::GetTriangleArea per triangle: 0.5 * |(p0 - p1) x (p0 - p2)| in float64, in tri_area's expression
    order (every product and sum rounded on its own: numpy never contracts)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = _tri(triangles)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    x, y = p0 - p1, p0 - p2
    c0 = x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1]
    c1 = x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2]
    c2 = x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]
    return 0.5 * np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)


def cluster_loop(triangles):
    """Open3D's loop: labels int32 [T], cluster sizes (list)"""
    t = _tri(triangles)
    keys = edge_keys(t)
    edges = {}
    for tidx in range(len(t)):
        for e in range(3):
            edges.setdefault((int(keys[tidx, e, 0]), int(keys[tidx, e, 1])), []).append(tidx)
    adjacency = [set() for _ in range(len(t))]
    for tidx in range(len(t)):
        for e in range(3):
            for nb in edges[(int(keys[tidx, e, 0]), int(keys[tidx, e, 1]))]:
                adjacency[tidx].add(nb)
    labels = np.full(len(t), -1, np.int32)
    sizes = []
    for tidx in range(len(t)):
        if labels[tidx] != -1:
            continue
        cluster = len(sizes)
        sizes.append(0)
        queue = deque([tidx])
        labels[tidx] = cluster
        while queue:
            cur = queue.popleft()
            sizes[cluster] += 1
            for nb in adjacency[cur]:
                if labels[nb] == -1:
                    queue.append(nb)
                    labels[nb] = cluster
    return labels, sizes


def cluster_closed(triangles):
    """the closed form: labels int32 [T], cluster sizes (list)"""
    t = _tri(triangles)
    parent = list(range(len(t)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    k = edge_keys(t).reshape(-1, 2)
    order = np.lexsort((k[:, 1], k[:, 0]))
    k = k[order]
    owner = order // 3
    for i in range(1, len(k)):
        if k[i, 0] == k[i - 1, 0] and k[i, 1] == k[i - 1, 1]:
            a, b = find(int(owner[i])), find(int(owner[i - 1]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(len(t))], np.int64)
    # the smaller root always wins, so a root is its component's smallest triangle index
    roots = np.unique(root)
    labels = np.searchsorted(roots, root).astype(np.int32)
    return labels, np.bincount(labels, minlength=len(roots)).tolist() if len(t) else []


def cluster_connected_triangles(vertices, triangles):
    """(labels int32 [T], sizes int32 [C], terms): terms[k] = the areas of cluster k's triangles, ascending triangle
    index -- the terms of the device's sum (None without vertices)"""
    labels, sizes = cluster_closed(triangles)
    terms = None
    if vertices is not None:
        area = triangle_areas(vertices, triangles)
        terms = [area[labels == k] for k in range(len(sizes))]
    return labels, np.asarray(sizes, np.int32), terms


def area_bound(terms):
    """the issue's bound for one cluster: n * 2^-52 * fsum (any association of n non-negative terms errs by at most
    (n - 1) 2^-53 relative to first order; the factor 2 is the margin)"""
    s = math.fsum(terms.tolist())
    return s, len(terms) * 2.0 ** -52 * s


# ------------------------------------------------------------------------------------------------------ clean-up
def remove_triangles_by_mask(triangles, mask):
    t = _tri(triangles)
    mask = np.asarray(mask, bool).reshape(-1)
    if len(mask) != len(t):
        raise RuntimeError("[RemoveTrianglesByMask] triangle_mask needs to have same size as triangles_.")
    out = [t[i] for i in range(len(t)) if not mask[i]]
    return np.asarray(out, np.int32).reshape(-1, 3)


def remove_triangles_by_index(triangles, indices):
    t = _tri(triangles)
    mask = np.zeros(len(t), bool)
    for i in indices:
        if 0 <= i < len(t):
            mask[i] = True
    return remove_triangles_by_mask(t, mask)


def degenerate_mask(triangles):
    t = _tri(triangles)
    return np.array([a == b or b == c or a == c for a, b, c in t.tolist()], bool).reshape(-1)


def remove_degenerate_triangles(triangles):
    return remove_triangles_by_mask(triangles, degenerate_mask(triangles))


def canonical_key(t0, t1, t2):
    """Open3D's RemoveDuplicatedTriangles key"""
    if t0 <= t1:
        return (t0, t1, t2) if t0 <= t2 else (t2, t0, t1)
    return (t1, t2, t0) if t1 <= t2 else (t2, t0, t1)


def duplicated_mask(triangles):
    t = _tri(triangles)
    seen = {}
    mask = np.zeros(len(t), bool)
    for i, (a, b, c) in enumerate(t.tolist()):
        k = canonical_key(a, b, c)
        if k in seen:
            mask[i] = True
        else:
            seen[k] = i
    return mask


def remove_duplicated_triangles(triangles):
    return remove_triangles_by_mask(triangles, duplicated_mask(triangles))


def remove_unreferenced_vertices(vertices, triangles, colors=None, normals=None):
    """(vertices', triangles', colors', normals', kept old index int32)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = _tri(triangles)
    used = np.zeros(len(v), bool)
    for row in t.tolist():
        for i in row:
            used[i] = True
    new = np.full(len(v), -1, np.int64)
    kept = []
    for i in range(len(v)):
        if used[i]:
            new[i] = len(kept)
            kept.append(i)
    kept = np.asarray(kept, np.int32)
    t2 = np.asarray([[new[i] for i in row] for row in t.tolist()], np.int32).reshape(-1, 3)
    sel = lambda a: None if a is None else np.asarray(a, np.float64).reshape(-1, 3)[kept]  # noqa: E731
    return v[kept], t2, sel(colors), sel(normals), kept
