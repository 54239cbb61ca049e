"""Designed meshes for the mesh-component tests (tests/test_mesh_components_api.py on the CPU, which asserts that each
is what it claims to be; tests/test_gpu_mesh_components.py on the GPU).  numpy only, fixed seeds, at most about 5 000
triangles each.  A builder returns int32 triangles [T][3], and float64 vertices [V][3] where areas matter."""
import numpy as np

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def _i32(t):
    return np.ascontiguousarray(np.asarray(t, np.int32).reshape(-1, 3))


def vertex_count(tri):
    return int(tri.max()) + 1 if len(tri) else 0


def random_vertices(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


# ------------------------------------------------------------------------------------------------- random soups
def soup(seed):
    """1 .. 6 groups of triangles, each group drawing its indices from its own few vertices (3 .. 14): non-manifold
    edges, degenerate and duplicated triangles all occur, and the groups are separate clusters at least; shuffled"""
    rng = np.random.default_rng(seed)
    groups = int(rng.integers(1, 7))
    tris, base = [], 0
    budget = int(rng.integers(1, 501))
    for g in range(groups):
        nv = int(rng.integers(3, 15))
        nt = max(1, budget // groups + int(rng.integers(-3, 4)))
        tris.append(base + rng.integers(0, nv, (nt, 3)))
        base += nv
    t = np.concatenate(tris)[:500]
    return _i32(t[rng.permutation(len(t))])


def random_soups(seed0, count=60):
    return [soup(seed0 * 1000 + i) for i in range(count)]


# ------------------------------------------------------------------------------------------------- connectivity
def bow_tie():
    """two triangles sharing vertex 2 only: two clusters"""
    return _i32([[0, 1, 2], [2, 3, 4]])


def bow_tie_fan(n=100):
    """n triangles round vertex 0, no two sharing an edge: n clusters"""
    return _i32([[0, 2 * k + 1, 2 * k + 2] for k in range(n)])


def opposite_edges():
    """(1, 2) once as 1 -> 2 and once as 2 -> 1 (a consistently oriented pair), then a pair sharing 5 -> 6 in the same
    direction (inconsistently oriented), then a lone triangle: clusters 0, 0, 1, 1, 2"""
    return _i32([[0, 1, 2], [2, 1, 3], [4, 5, 6], [5, 6, 7], [8, 9, 10]])


def shared_edge(k):
    """k triangles on the one edge (0, 1): one cluster"""
    return _i32([[0, 1, 2 + j] for j in range(k)])


NM_FILL, NM_RUN = 34, 300
NM_EDGES = ((102, 103), (104, 105))


def nonmanifold_runs():
    """34 lone triangles on vertices 0 .. 101 (102 keys ahead of everything else), then 300 triangles on the edge
    (102, 103) and 300 on (104, 105): in the sorted key array the run of (102, 103) is positions 102 .. 401, across
    256, and the run of (104, 105) is 1002 .. 1301, across 1024.  36 clusters."""
    t = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(NM_FILL)]
    t += [[102, 103, 106 + j] for j in range(NM_RUN)]
    t += [[104, 105, 106 + NM_RUN + j] for j in range(NM_RUN)]
    return _i32(t)


def degenerate_links():
    """(a, a, b) and (a, a, c) connect through the key (a, a), and so does (a, a, a); (d, d, d) is alone; (e, f, e)
    has the keys (e, f) twice and (e, e)"""
    return _i32([[5, 5, 1], [7, 8, 9], [5, 5, 2], [5, 5, 5], [3, 3, 3], [10, 11, 10], [10, 10, 12]])


DEGENERATE_LINK_LABELS = [0, 1, 0, 0, 2, 3, 3]


def strip(n=4096):
    """triangle t = (t, t + 1, t + 2): each shares an edge with the next only"""
    return _i32([[t, t + 1, t + 2] for t in range(n)])


def two_strips(n=2048):
    """two strips on separate vertices, their triangles interleaved: labels 0, 1, 0, 1, ..."""
    a = strip(n)
    b = a + (n + 2)
    return _i32(np.stack([a, b], axis=1).reshape(-1, 3))


def numbering():
    """the cluster that holds vertex 0 holds only the last two triangles: numbered by smallest triangle index it is
    cluster 1, by smallest vertex index it would be cluster 0"""
    return _i32([[3, 4, 5], [4, 5, 6], [0, 1, 2], [1, 2, 7]])


def isolated(n):
    """n triangles with three vertices each of their own"""
    return _i32(np.arange(3 * n).reshape(n, 3))


# -------------------------------------------------------------------------------------------------------- areas
def isolated_with_areas(n, seed=7):
    """isolated(n) with vertices: random triangles, and among the first few a zero-area one (three equal points), a
    collinear one, one with denormal edges and one whose cross product underflows"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-2.0, 2.0, (3 * n, 3)) * 10.0 ** rng.integers(-3, 3, (3 * n, 1))
    special = [
        np.array([[1.0, 2.0, 3.0]] * 3),
        np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]),
        np.array([[0.0, 0.0, 0.0], [5e-324, 0.0, 0.0], [0.0, 1.5e-323, 0.0]]),
        np.array([[1.0, 1.0, 1.0], [1.0 + 1e-160, 1.0, 1.0], [1.0, 1.0 + 1e-170, 1.0]]),
        np.array([[0.0, 0.0, 0.0], [1e-200, 0.0, 0.0], [0.0, 1e-200, 0.0]]),
    ]
    for i, s in enumerate(special[:n]):
        v[3 * i:3 * i + 3] = s
    return v, isolated(n)


def area_fan(n=4096, seed=11):
    """n triangles on the edge (0, 1) of length 2, apex j at height h_j above it: areas h_j, spread log-uniformly over
    1e-12 .. 1e3 in a shuffled order.  One cluster."""
    rng = np.random.default_rng(seed)
    h = 10.0 ** rng.uniform(-12.0, 3.0, n)
    h[0], h[1] = 1e-12, 1e3
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    v = np.zeros((n + 2, 3))
    v[0], v[1] = (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    v[2:, 0] = rng.uniform(-1.0, 1.0, n)
    v[2:, 1] = h * np.cos(ang)
    v[2:, 2] = h * np.sin(ang)
    return v, shared_edge(n)


# --------------------------------------------------------------------------------------------------- duplicates
def duplicate_basics():
    """rotations, a flip, the (a, b, a) quirk, survivors that are not in canonical rotation"""
    return _i32([
        [2, 0, 1],   # 0 kept: first of its rotations, not the canonical one
        [0, 1, 2],   # 1 removed (rotation of 0)
        [1, 2, 0],   # 2 removed
        [0, 2, 1],   # 3 kept: the flip
        [2, 1, 0],   # 4 removed (rotation of the flip)
        [3, 7, 3],   # 5 kept: (a, b, a), key (3, 7, 3)
        [3, 3, 7],   # 6 kept: key (3, 3, 7)
        [7, 3, 3],   # 7 removed: key (3, 3, 7) too
        [9, 4, 6],   # 8 kept: key (4, 6, 9)
        [6, 9, 4],   # 9 removed
        [5, 5, 5],   # 10 kept
        [5, 5, 5],   # 11 removed
    ])


DUPLICATE_BASICS_REMOVED = [1, 2, 4, 7, 9, 11]


def duplicate_runs(n, seed=13):
    """n triangles drawn (with repeats, in random rotations) from n // 4 + 1 distinct ones: runs of 3 and more equal
    keys, spread over the whole array, crossing every block boundary there is"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 40, (n // 4 + 1, 3))
    pick = base[rng.integers(0, len(base), n)]
    rot = rng.integers(0, 3, n)
    return _i32(np.stack([np.roll(p, r) for p, r in zip(pick, rot)]))


BIG_NV = 2 ** 31 - 1
_TOP = 2 ** 30  # the top bit of a 31-bit index


def big_index_duplicates():
    """indices up to 2^31 - 2 (n_vertices = 2^31 - 1, no vertex array): keys that differ only in the third component,
    only in the first, only in the top bit of one index -- none of them duplicates -- among true duplicates.  A dropped
    sort pass or a narrow key merges or separates the wrong ones.  Every key is written in canonical rotation."""
    m = BIG_NV - 1
    rows = []
    for top in (0, _TOP):
        rows += [[5, 9 + top, 17 + top], [5, 9 + top, 18 + top]]           # third component only
        rows += [[6, 700 + top, 900 + top], [7, 700 + top, 900 + top]]     # first component only
    rows += [[3, 4, 5], [3, 4, 5 + _TOP], [3, 4 + _TOP, 5], [3 + _TOP, 4 + _TOP, 5 + _TOP]]  # top bits only
    rows += [[1, m, m - 1], [1, m, m - 2], [0, m, m], [0, 0, m]]
    first = _i32(rows)
    rng = np.random.default_rng(17)
    again = first[rng.integers(0, len(first), 3 * len(first))]             # true duplicates, in rotations
    again = np.stack([np.roll(p, int(r)) for p, r in zip(again, rng.integers(0, 3, len(again)))])
    t = np.concatenate([first, again])
    # 300 fillers so that the runs cross the 256 boundary, then everything shuffled
    fill = np.stack([np.arange(300) * 3 + 100, np.arange(300) * 3 + 101 + _TOP, np.arange(300) * 3 + 102], axis=1)
    t = np.concatenate([t, fill])
    return _i32(t[rng.permutation(len(t))]), len(first) + 300


def big_index_edges():
    """the same large indices for the clustering's edge keys: pairs of triangles whose edges differ only in the top bit
    of one index (not adjacent) beside pairs that share such an edge (adjacent)"""
    m = BIG_NV - 1
    t = [
        [10, 20, 30], [10 + _TOP, 20, 31],          # (10, 20) vs (20, 10 + top): apart
        [40, 50, 60], [40, 50 + _TOP, 61],          # (40, 50) vs (40, 50 + top): apart
        [70 + _TOP, 80 + _TOP, 90], [80 + _TOP, 70 + _TOP, 91],   # share (70 + top, 80 + top)
        [m, m - 1, 5], [m - 1, m, 6],               # share (m - 1, m)
        [m, 100, 101], [m - _TOP, 100, 102],        # (100, m) vs (100, m - top): apart
        [0, m, 200], [m, 0, 201],                   # share (0, m)
    ]
    return _i32(t)


BIG_INDEX_EDGE_LABELS = [0, 1, 2, 3, 4, 4, 5, 5, 6, 7, 8, 8]


# ---------------------------------------------------------------------------------------------------- compaction
def masks(n):
    """name -> bool mask of length n"""
    out = {"all false": np.zeros(n, bool), "all true": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}
    first = np.ones(n, bool)
    first[0] = False
    last = np.ones(n, bool)
    last[-1] = False
    out["only the first survives"] = first
    out["only the last survives"] = last
    return out


def cleanup_soup(n, seed=19):
    """n triangles over few vertices (degenerate, duplicated and clean ones), on n + 7 vertices of which many are
    unreferenced, the last one referenced"""
    rng = np.random.default_rng(seed + n)
    nv = n + 7
    t = rng.integers(0, max(3, min(nv, 12 + n // 8)), (n, 3)) * 3 % nv
    t[-1] = (nv - 1, 0, 3 % nv)
    return nv, _i32(t)


# ------------------------------------------------------------------------------------------------ a two-part volume
def two_spheres():
    """a 2 x 2 x 2 unit block (tests/mc_volumes.py layout) holding two separate spheres, a large one and a small one:
    (keys, tsdf, weight, colour)"""
    import mc_volumes as MV

    g = np.indices((32, 32, 32)).astype(np.float64)
    def sdf(c, r):
        return np.sqrt(((g - np.array(c, np.float64).reshape(3, 1, 1, 1)) ** 2).sum(0)) - r
    d = np.minimum(sdf((12.3, 13.1, 14.2), 8.4), sdf((25.2, 25.7, 24.9), 3.3))
    tsdf = np.clip(d / 4.0, -1.0, 1.0).astype(np.float32)
    weight = np.ones((32, 32, 32), np.float32)
    color = np.random.default_rng(23).uniform(0.0, 255.0, (32, 32, 32, 3))
    return MV.split(MV.BLOCK_KEYS, (-1, -1, -1), tsdf, weight, color)
