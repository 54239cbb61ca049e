"""Designed triangle meshes for tests/test_gpu_mesh_edges.py (numpy only): what a marching-cubes mesh of a scan --
manifold, valence <= ~12, every vertex referenced, no degenerate triangle, triangles of similar area -- never gives.
Every builder returns (V float64 [nv][3], T int32 [nt][3]) from a fixed seed."""
import numpy as np


def fan(n=20000, seed=1):
    """one hub in n triangles with random rim positions: the hub's normal is one long serial sum, so any reordering
    of its terms changes the bits"""
    rng = np.random.default_rng(seed)
    V = np.concatenate([[[0.1, -0.2, 0.3]], rng.uniform(-1, 1, (n + 1, 3))])
    i = np.arange(n)
    return V, np.stack([np.zeros(n, np.int64), i + 1, i + 2], 1).astype(np.int32)


def unreferenced(seed=2):
    """vertices that no triangle references at the start, in the middle and at the end"""
    rng = np.random.default_rng(seed)
    nv = 700
    V = rng.uniform(-1, 1, (nv, 3))
    used = np.concatenate([np.arange(5, 300), np.arange(311, 690)])
    return V, rng.choice(used, (1500, 3)).astype(np.int32)


def single(nv, seed=3):
    """one triangle among nv vertices (nv around the 256-vertex block)"""
    rng = np.random.default_rng(seed + nv)
    V = rng.uniform(-1, 1, (nv, 3))
    t = (0, 0, 0) if nv < 3 else (nv - 1, 0, nv // 2)
    return V, np.array([t], np.int32)


def repeated_corners(seed=4):
    """triangles (a, a, b) and (a, a, a) among ordinary ones: a vertex gets the same triangle's normal two or three
    times, and that normal is zero"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1, 1, (40, 3))
    T = rng.integers(0, 40, (200, 3))
    T[::7, 1] = T[::7, 0]
    T[::21, 2] = T[::21, 0]
    T[-1] = (39, 39, 39)
    return V, T.astype(np.int32)


def underflow(seed=5):
    """coordinates ~1e-90: the triangle normals are ~1e-180, their squared length underflows to 0 and Open3D leaves
    the sum unnormalised; the second half of the mesh is at ordinary scale"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1, 1, (300, 3))
    V[:150] *= 1e-90
    T = np.concatenate([rng.integers(0, 150, (400, 3)), rng.integers(150, 300, (400, 3))])
    return V, T.astype(np.int32)


def opposite():
    """two opposite triangles on the same vertices: every normal sum is exactly zero"""
    V = np.array([[0.3, 0.1, 0.0], [1.7, 0.2, 0.5], [0.4, 1.9, -0.6], [5.0, 5.0, 5.0]])
    return V, np.array([[0, 1, 2], [0, 2, 1]], np.int32)


def ties():
    """four right triangles with legs 1: areas and CDF exact (0.25, 0.5, 0.75, 1), so cdf * N is an exact .5 tie for
    N = 2, 6, 10, where rounding half away from zero (Open3D's std::round) and half to even disagree"""
    V, T = [], []
    for k in range(4):
        o = np.array([4.0 * k, 2.0 * (k & 1), 8.0 - k])
        V += [o, o + [1.0, 0, 0], o + [0, 1.0, 0]]
        T.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.array(V), np.array(T, np.int32)


ZERO_RUN = 9000


def zero_area(seed=6):
    """zero-area triangles (a repeated corner, or three exactly collinear points) singly and in a run of ZERO_RUN
    between positive ones: their cumulative counts tie, and the run is longer than the counts the fused sampler stages"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1, 1, (64, 3))
    V[61] = V[60] * 2.0  # 0, V[60], 2 V[60] collinear exactly
    V[62] = 0.0
    pos = rng.integers(0, 60, (12, 3))
    pos[:, 1] = (pos[:, 0] + 1 + pos[:, 1] % 20) % 60
    pos[:, 2] = (pos[:, 0] + 25 + pos[:, 2] % 20) % 60
    run = np.stack([rng.integers(0, 60, ZERO_RUN)] * 2 + [rng.integers(0, 60, ZERO_RUN)], 1)
    run[::3] = (62, 60, 61)
    T = np.concatenate([[(3, 3, 9)], pos[0:1], [(62, 60, 61)], pos[1:3], [(7, 8, 7)], pos[3:6], run, pos[6:9],
                        [(5, 5, 5)], pos[9:12], [(62, 61, 60)]])
    return V, T.astype(np.int32)


def tiny(n=300000, seed=7):
    """n small triangles along a random walk: with a few hundred points every 256-point tile spans far more triangles
    than the fused sampler stages"""
    rng = np.random.default_rng(seed)
    V = np.cumsum(rng.uniform(-1e-3, 1e-3, (n + 2, 3)), 0)
    i = np.arange(n)
    return V, np.stack([i, i + 1, i + 2], 1).astype(np.int32)


def one_triangle():
    return np.array([[0.0, 0.0, 1.0], [2.0, 0.5, -1.0], [0.25, 3.0, 0.5]]), np.array([[2, 0, 1]], np.int32)


def two_triangles():
    V = np.array([[0.0, 0.0, 1.0], [2.0, 0.5, -1.0], [0.25, 3.0, 0.5], [-1.0, -1.0, 0.125]])
    return V, np.array([[2, 0, 1], [0, 3, 1]], np.int32)


def skew(seed=8):
    """one triangle 10^6 times larger (in area) than each of 1000 others, in the middle of them"""
    rng = np.random.default_rng(seed)
    small = rng.uniform(-1e-3, 1e-3, (1000, 3, 3)) + rng.uniform(-1, 1, (1000, 1, 3))
    big = rng.uniform(-1e-3, 1e-3, (1, 3, 3)) * 1e3
    tri = np.concatenate([small[:500], big, small[500:]])
    return tri.reshape(-1, 3), np.arange(3 * 1001).reshape(-1, 3).astype(np.int32)


NORMALS = {"fan": fan, "unreferenced": unreferenced, "repeated_corners": repeated_corners, "underflow": underflow,
           "opposite": opposite, "zero_area": zero_area, "ties": ties}
NORMALS.update({f"single_{nv}": (lambda nv=nv: single(nv)) for nv in (1, 3, 255, 256, 257)})

# mesh -> the n_points it is sampled with
SAMPLING = {"ties": (ties, (2, 6, 10)),
            "zero_area": (zero_area, (1, 13, 257, 1000, 20000)),
            "tiny": (tiny, (1, 2, 255, 256, 257, 1000)),
            "one_triangle": (one_triangle, (100000,)),
            "two_triangles": (two_triangles, (100000,)),
            "skew": (skew, (1000, 100000))}
