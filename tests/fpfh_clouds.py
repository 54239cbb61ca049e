"""The designed clouds of the FPFH tests (tests/test_fpfh_ref.py on the host, tests/test_gpu_fpfh.py on the device) and
their references, each computed once.  Normals are generic (random unit vectors, or exact normals plus 5 % noise,
renormalised) so that no comparison of fpfh_ref's fragile kind is nearly a tie; the two clouds that are all ties
(exact radial normals, axis-aligned normals) exist to show the flag."""
import functools

import numpy as np

import fpfh_ref as FR

WORKGROUP_POINTS = 64  # csrc/features.hip: points per workgroup of the list, SPFH and FPFH kernels


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def random_normals(n, seed):
    return unit(np.random.default_rng(seed).normal(size=(n, 3)))


def noisy(normals, seed):
    return unit(normals + 0.05 * np.random.default_rng(seed).normal(size=normals.shape))


def lattice(m=7, spacing=0.125):
    g = np.arange(m) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def sphere(n=700, radius=0.1, seed=3):
    d = random_normals(n, seed)
    return d * radius, d


def planar(m=12, seed=5):
    """a jittered m x m grid in the plane z = 0 with normals (0, 0, 1)"""
    g = np.arange(m) * 0.01
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    xy = xy + np.random.default_rng(seed).uniform(-0.002, 0.002, xy.shape)
    P = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)
    return P, np.broadcast_to([0.0, 0.0, 1.0], P.shape).copy()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, normals, k, radius or None)"""
    rng = np.random.default_rng(11)
    c = {}
    P600, N600 = rng.random((600, 3)), random_normals(600, 12)
    c["random_k20"] = (P600, N600, 20, None)
    c["lattice_k27"] = (lattice(), random_normals(343, 13), 27, None)  # distance ties: the canonical order decides
    S, SN = sphere()
    c["sphere_hybrid_k100"] = (S, noisy(SN, 14), 100, 0.06)  # lists of mixed length, some longer than 64
    for k in (64, 65, 128):  # both sides of the list-storage boundary, and the longest list
        c[f"random_k{k}"] = (P600, N600, k, None)
    sites = rng.random((60, 3))
    c["coincident_k9"] = (np.repeat(sites, 4, axis=0), random_normals(240, 15), 9, None)
    far = np.concatenate([rng.random((100, 3)) * 0.05, [[10.0, 10.0, 10.0]]])
    c["far_point_hybrid_k16"] = (far, random_normals(101, 16), 16, 0.03)
    t = np.sort(rng.random(150))
    c["line_k10"] = (t[:, None] * np.array([0.3, 0.5, 0.7]), random_normals(150, 17), 10, None)
    c["n1_k20"] = (rng.random((1, 3)), random_normals(1, 18), 20, None)
    c["n2_k20"] = (rng.random((2, 3)), random_normals(2, 19), 20, None)
    c["n5_k20"] = (rng.random((5, 3)), random_normals(5, 20), 20, None)
    for n in (2 * WORKGROUP_POINTS - 1, 2 * WORKGROUP_POINTS, 2 * WORKGROUP_POINTS + 1):
        c[f"n{n}_k10"] = (rng.random((n, 3)), random_normals(n, 21), 10, None)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    P, N, k, radius = cases()[name]
    return FR.compute(P, N, k, radius)
