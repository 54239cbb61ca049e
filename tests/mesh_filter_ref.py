"""numpy restatement of the mesh filters (DESIGN.md §4 "mesh filters"): the adjacency list, filter_smooth_simple /
_laplacian / _taubin, filter_sharpen and simplify_vertex_clustering (Average).  Every operator is stated twice: a
literal per-vertex Python loop over sorted sets (the definition, `*_loop`), and a vectorised form that walks the
neighbour rank k over all vertices at once (`acc[deg > k] += x[nbr[:, k]]`; rows of more than HEAVY neighbours by an
in-order cumulative sum each), which performs the same float64
operations in the same order per vertex and is fast enough for the GPU tests.  tests/test_mesh_filter_api.py asserts
that the two agree bit for bit.  numpy only; also the designed meshes of the filter tests."""
import math

import numpy as np

INT_MAX = 2147483647
SIMPLE, LAPLACIAN, TAUBIN, SHARPEN = "simple", "laplacian", "taubin", "sharpen"
SCOPES = ("All", "Color", "Normal", "Vertex")


def _i32(t):
    return np.ascontiguousarray(np.asarray(t, np.int32).reshape(-1, 3))


# ---------------------------------------------------------------------------------------------------- adjacency
def check_indices(tri, nv, who):
    tri = np.asarray(tri).reshape(-1, 3)
    if len(tri) and (tri.min() < 0 or tri.max() >= nv):
        raise RuntimeError(f"[{who}] triangle index out of range [0, n_vertices)")


def adjacency_loop(tri, nv):
    """the definition: a list of sets"""
    check_indices(tri, nv, "ComputeAdjacencyList")
    adj = [set() for _ in range(nv)]
    for a, b, c in np.asarray(tri).reshape(-1, 3).tolist():
        adj[a].add(b)
        adj[a].add(c)
        adj[b].add(a)
        adj[b].add(c)
        adj[c].add(a)
        adj[c].add(b)
    return adj


def csr_of_sets(adj):
    offsets = np.zeros(len(adj) + 1, np.int32)
    nbr = []
    for v, s in enumerate(adj):
        nbr += sorted(s)
        offsets[v + 1] = len(nbr)
    return offsets, np.asarray(nbr, np.int32).reshape(-1)


def adjacency_csr(tri, nv):
    """the same as a CSR (offsets int32 [nv + 1], neighbours int32 [E], rows ascending), vectorised"""
    check_indices(tri, nv, "ComputeAdjacencyList")
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    src = np.concatenate([a, a, b, b, c, c])
    dst = np.concatenate([b, c, a, c, a, b])
    keys = np.unique(src * max(nv, 1) + dst)
    v, w = keys // max(nv, 1), keys % max(nv, 1)
    offsets = np.searchsorted(v, np.arange(nv + 1)).astype(np.int32)
    return offsets, w.astype(np.int32)


HEAVY = 32  # rows longer than this are summed one vertex at a time (an in-order cumulative sum)


def padded(offsets, nbr):
    """(deg [nv], table [nv][<= HEAVY], heavy) of a CSR: the rows of at most HEAVY neighbours as a table, short rows
    padded with 0 (deg counts the table's entries: 0 for a heavy row), and the longer rows as a list of
    (vertex, its neighbours)"""
    offsets = np.asarray(offsets, np.int64)
    nbr = np.asarray(nbr, np.int64)
    full = np.diff(offsets)
    heavy = [(int(v), nbr[offsets[v]:offsets[v + 1]]) for v in np.nonzero(full > HEAVY)[0]]
    deg = np.where(full > HEAVY, 0, full)
    width = int(deg.max()) if len(deg) and deg.max() > 0 else 0
    table = np.zeros((len(deg), width), np.int64)
    if width:
        light = np.repeat(full <= HEAVY, full)
        rank = (np.arange(len(nbr)) - np.repeat(offsets[:-1], full))[light]
        table[np.repeat(np.arange(len(deg)), deg), rank] = nbr[light]
    return deg, table, heavy


# ------------------------------------------------------------------------------------------------------ filters
def _filtered(scope, V, N, C):
    """name -> array of the attributes a filter changes"""
    assert scope in SCOPES
    out = {}
    if scope in ("All", "Vertex"):
        out["V"] = V
    if scope in ("All", "Normal") and N is not None:
        out["N"] = N
    if scope in ("All", "Color") and C is not None:
        out["C"] = C
    return out


def _step_loop(kind, par, P, X, adj):
    """one step of one attribute X [nv][3], literally; P: the positions of the previous step (Laplacian weights)"""
    out = X.copy()
    for v, s in enumerate(adj):
        nb = sorted(s)
        n = len(nb)
        if n == 0:
            continue  # an isolated vertex keeps its attributes (deliberate deviation from Open3D)
        for d in range(3):
            x0 = float(X[v, d])
            if kind == SIMPLE:
                acc = x0
                for w in nb:
                    acc = acc + float(X[w, d])
                out[v, d] = acc / float(1 + n)
            elif kind == SHARPEN:
                acc = 0.0
                for w in nb:
                    acc = acc + float(X[w, d])
                out[v, d] = x0 * (1.0 + par * float(n)) - par * acc
            else:
                W, S = 0.0, 0.0
                for w in nb:
                    dx, dy, dz = (float(P[v, i]) - float(P[w, i]) for i in range(3))
                    dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
                    wt = 1.0 / (dist + 1e-12)
                    W = W + wt
                    S = S + wt * float(X[w, d])
                out[v, d] = x0 + par * (S / W - x0)
    return out


def _chain(first, terms):
    """((first + terms[0]) + terms[1]) + ... along axis 0: numpy's accumulate adds strictly in order"""
    return np.add.accumulate(np.concatenate([np.reshape(first, (1,) + terms.shape[1:]), terms]), axis=0)[-1]


def _weight(pv, pw):
    d = pv - pw
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return 1.0 / (dist + 1e-12)


def _step_vec(kind, par, P, attrs, deg, table, heavy, full_deg):
    """one step of every attribute of `attrs` (name -> [nv][3]), vectorised over the vertices"""
    iso = full_deg == 0
    n = full_deg.astype(np.float64)[:, None]
    out = {}
    if kind == LAPLACIAN:
        W = np.zeros(len(deg))
        per_rank = []
        for k in range(table.shape[1]):
            m = deg > k
            w = table[m, k]
            wt = _weight(P[m], P[w])
            W[m] += wt
            per_rank.append((m, w, wt))
        heavy_wt = [_weight(P[v][None, :], P[w]) for v, w in heavy]
        for (v, w), wt in zip(heavy, heavy_wt):
            W[v] = _chain(0.0, wt)
        for name, X in attrs.items():
            S = np.zeros_like(X)
            for m, w, wt in per_rank:
                S[m] += wt[:, None] * X[w]
            for (v, w), wt in zip(heavy, heavy_wt):
                S[v] = _chain(np.zeros(3), wt[:, None] * X[w])
            with np.errstate(invalid="ignore", divide="ignore"):
                r = X + par * (S / W[:, None] - X)
            r[iso] = X[iso]
            out[name] = r
        return out
    for name, X in attrs.items():
        acc = X.copy() if kind == SIMPLE else np.zeros_like(X)
        for k in range(table.shape[1]):
            m = deg > k
            acc[m] += X[table[m, k]]
        for v, w in heavy:
            acc[v] = _chain(acc[v], X[w])
        r = acc / (1.0 + n) if kind == SIMPLE else X * (1.0 + par * n) - par * acc
        r[iso] = X[iso]
        out[name] = r
    return out


def _steps(kind, iterations, p0, p1):
    if iterations <= 0:
        return []
    if kind == TAUBIN:
        return [(LAPLACIAN, p0), (LAPLACIAN, p1)] * iterations
    return [(kind, p0)] * iterations


def _f64(a):
    return None if a is None else np.array(a, np.float64).reshape(-1, 3)


def filter_mesh(kind, V, tri, N=None, C=None, iterations=1, p0=0.5, p1=-0.53, scope="All", loop=False):
    """(V', N', C') of filter_smooth_simple (kind SIMPLE), filter_smooth_laplacian (LAPLACIAN, p0 = lambda),
    filter_smooth_taubin (TAUBIN, p0 = lambda, p1 = mu) or filter_sharpen (SHARPEN, p0 = strength); attributes outside
    the scope, or absent, come back as copies (None stays None)."""
    V, N, C = _f64(V), _f64(N), _f64(C)
    cur = {"V": V, "N": N, "C": C}
    names = list(_filtered(scope, V, N, C))
    if loop:
        adj = adjacency_loop(tri, len(V))
    else:
        offsets, nbr = adjacency_csr(tri, len(V))
        deg, table, heavy = padded(offsets, nbr)
        full_deg = np.diff(offsets)
    for step_kind, par in _steps(kind, iterations, p0, p1):
        P = cur["V"]
        if loop:
            new = {name: _step_loop(step_kind, par, P, cur[name], adj) for name in names}
        else:
            new = _step_vec(step_kind, par, P, {name: cur[name] for name in names}, deg, table, heavy, full_deg)
        cur.update(new)
    return cur["V"], cur["N"], cur["C"]


# --------------------------------------------------------------------------------------------------- clustering
def voxel_keys(V, voxel_size):
    """int64 [nv][3]: floor((p - (min_bound - vs / 2)) / vs) in float64, after VoxelDownSample's refusals"""
    vs = float(voxel_size)
    if not vs > 0.0:
        raise RuntimeError("[SimplifyVertexClustering] voxel_size <= 0.")
    vmin = V.min(0) - vs * 0.5
    vmax = V.max(0) + vs * 0.5
    if vs * float(INT_MAX) < float((vmax - vmin).max()):
        raise RuntimeError("[SimplifyVertexClustering] voxel_size is too small.")
    return np.floor((V - vmin) / vs).astype(np.int64)


def _rotate_min_first(a, b, c):
    if b < a and b <= c:
        return b, c, a
    if c < a and c < b:
        return c, a, b
    return a, b, c


def simplify_vertex_clustering_loop(V, tri, voxel_size, N=None, C=None):
    """the definition: (V', T', N', C')"""
    V, N, C = _f64(V), _f64(N), _f64(C)
    tri = _i32(tri)
    if len(V) == 0:
        return V, tri, N, C
    check_indices(tri, len(V), "SimplifyVertexClustering")
    keys = voxel_keys(V, voxel_size)
    index, members = {}, []
    newidx = np.zeros(len(V), np.int64)
    for v, k in enumerate(map(tuple, keys.tolist())):
        if k not in index:
            index[k] = len(members)
            members.append([])
        members[index[k]].append(v)  # ascending old index
        newidx[v] = index[k]

    def average(X):
        if X is None:
            return None
        out = np.zeros((len(members), 3))
        for j, vs in enumerate(members):
            for d in range(3):
                acc = 0.0
                for v in vs:
                    acc = acc + float(X[v, d])
                out[j, d] = acc / float(len(vs))
        return out

    seen, T = set(), []
    for a, b, c in newidx[tri.astype(np.int64)].reshape(-1, 3).tolist():
        if a == b or b == c or a == c:
            continue
        r = _rotate_min_first(a, b, c)
        if r not in seen:
            seen.add(r)
            T.append(r)
    return average(V), _i32(T), average(N), average(C)


def simplify_vertex_clustering(V, tri, voxel_size, N=None, C=None):
    """the same, vectorised: (V', T', N', C')"""
    V, N, C = _f64(V), _f64(N), _f64(C)
    tri = _i32(tri)
    if len(V) == 0:
        return V, tri, N, C
    check_indices(tri, len(V), "SimplifyVertexClustering")
    keys = voxel_keys(V, voxel_size)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))  # voxels by first appearance
    newidx = rank[inverse]
    K = len(first)
    order = np.argsort(newidx, kind="stable")  # grouped by new index, ascending old index inside a group
    count = np.bincount(newidx, minlength=K)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])

    def average(X):
        if X is None:
            return None
        acc = np.zeros((K, 3))
        for k in range(int(count.max())):
            m = count > k
            acc[m] += X[order[start[m] + k]]
        return acc / count.astype(np.float64)[:, None]

    M = newidx[tri.astype(np.int64)].reshape(-1, 3)
    M = M[~((M[:, 0] == M[:, 1]) | (M[:, 1] == M[:, 2]) | (M[:, 0] == M[:, 2]))]
    if len(M):
        a, b, c = M[:, 0], M[:, 1], M[:, 2]
        at_b = (b < a) & (b <= c)
        at_c = ~at_b & (c < a) & (c < b)
        R = np.where(at_b[:, None], np.stack([b, c, a], 1), np.where(at_c[:, None], np.stack([c, a, b], 1), M))
        _, keep = np.unique(R, axis=0, return_index=True)
        R = R[np.sort(keep)]  # one per distinct triple, in the order of their first source triangles
    else:
        R = M
    return average(V), _i32(R), average(N), average(C)


# ---------------------------------------------------------------------------------------------- designed meshes
def hub_fan(n=4096):
    """a closed fan round vertex 0 over the rim 1 .. n: (0, k + 1, k + 2) for k = 0 .. n - 2 and (0, n, 1).  Vertex 0
    has degree n, every rim vertex degree 3"""
    t = [[0, k + 1, k + 2] for k in range(n - 1)] + [[0, n, 1]]
    return _i32(t)


def hub_fan_vertices(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    ang = np.arange(n) * (2.0 * np.pi / n)
    r = 1.0 + 0.1 * rng.standard_normal(n)
    v = np.zeros((n + 1, 3))
    v[0] = (0.013, -0.021, 0.3)
    v[1:, 0], v[1:, 1], v[1:, 2] = r * np.cos(ang), r * np.sin(ang), 0.05 * rng.standard_normal(n)
    return v


def grid_mesh(nx=33, ny=33, seed=5, noise=0.01):
    """(V, T) of an nx x ny height field with noise: 2 (nx - 1)(ny - 1) triangles, interior degree 6"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * 0.05, np.arange(ny) * 0.05, indexing="ij")
    z = 0.2 * np.sin(3.0 * gx) * np.cos(2.0 * gy)
    V = np.stack([gx, gy, z], -1).reshape(-1, 3) + noise * rng.standard_normal((nx * ny, 3))
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    T = np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)])
    return V, _i32(T)


def attributes(nv, seed):
    """random normals (not unit) and colours for nv vertices"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, 3)), rng.uniform(0.0, 1.0, (nv, 3))


def with_isolated_vertices(seed=7):
    """the 9 x 9 grid mesh with 70 further vertices no triangle names, some in front, some at the end"""
    V, T = grid_mesh(9, 9, seed)
    rng = np.random.default_rng(seed)
    front, back = rng.uniform(-1.0, 1.0, (5, 3)), rng.uniform(-1.0, 1.0, (65, 3))
    return np.concatenate([front, V, back]), _i32(T + 5)


def coincident_neighbours(seed=9):
    """the 9 x 9 grid mesh with pairs and a triple of adjacent vertices at exactly the same point: distance 0, weight
    1e12"""
    V, T = grid_mesh(9, 9, seed)
    V[10] = V[11]
    V[40] = V[41]
    V[49] = V[41]  # 40, 41 and 49 (= 40 + 9) are mutually adjacent
    return V, T


def self_loops(seed=11):
    """the 9 x 9 grid mesh and degenerate triangles (a, a, b), (a, a, a): vertices that are their own neighbours"""
    V, T = grid_mesh(9, 9, seed)
    extra = _i32([[20, 20, 21], [33, 33, 33], [50, 60, 50]])
    return V, _i32(np.concatenate([T, extra]))


def tetrahedron():
    """small integer coordinates whose sum is divisible by 4: one simple step puts every vertex on the centroid"""
    V = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 8.0], [0.0, 8.0, 4.0], [8.0, 4.0, 0.0]])
    return V, _i32([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def unit_lattice(n=4):
    """the n^3 points of the unit lattice, x-major, and triangles (v, v + x, v + y) on it"""
    g = np.indices((n, n, n)).reshape(3, -1).T.astype(np.float64)
    idx = np.arange(n ** 3).reshape(n, n, n)
    T = np.stack([idx[:-1, :-1, :], idx[1:, :-1, :], idx[:-1, 1:, :]], -1).reshape(-1, 3)
    return g, _i32(T)
