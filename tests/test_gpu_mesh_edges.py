"""GPU parity of the mesh operators (mesh_ops.hip: compute_vertex_normals by the corner sort, get_surface_area,
sample_points_uniformly, its batch form and the fused sample_points_min_z) on the designed meshes of
tests/mesh_cases.py, bit for bit against the CPU oracle.  No volume is involved: the meshes
are built from arrays, so the normals take the corner sort.  Every comparison is assert_bitwise; there is no tolerance.

Left out on purpose: the rounding shortfall (k < n_points after the last triangle) and non-finite areas.  With finite
areas the last CDF value is within a few ulp of 1, so round(cdf * N) = N for these N and no shortfall occurs; NaN
payloads are not comparable bitwise."""
import numpy as np
import pytest

import mesh_cases as MC
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

SEEDS = (0, 2 ** 63 + 1)


def _mesh(pkg, V, T, VN=None, VC=None):
    m = pkg.geometry.TriangleMesh(V.copy(), T.copy())
    if VN is not None:
        m.vertex_normals = VN.copy()
    if VC is not None:
        m.vertex_colors = VC.copy()
    return m


@pytest.mark.parametrize("case", sorted(MC.NORMALS))
def test_vertex_normals_bitexact(pkg, O, gpu, case):
    V, T = MC.NORMALS[case]()
    rN = O.vertex_normals(V, T)
    mesh = _mesh(pkg, V, T)
    mesh.compute_vertex_normals()
    assert_bitwise(np.asarray(mesh.vertex_normals), rN, f"{case}: vertex normals")
    ref = np.zeros(len(V), bool)
    ref[T.reshape(-1)] = True
    if case == "unreferenced":
        assert not ref[:5].any() and not ref[300:311].any() and not ref[690:].any() and ref[5:300].all()
        assert not rN[~ref].any()
    if case == "underflow":
        sq = (rN[:, 0] * rN[:, 0] + rN[:, 1] * rN[:, 1]) + rN[:, 2] * rN[:, 2]
        assert (sq[:150] == 0).all() and rN[:150].any(1).all() and (sq[150:] > 0.5).all()  # left unnormalised
    if case == "opposite":
        assert not rN.any()
    if case == "fan":
        assert np.bincount(T.reshape(-1))[0] == 20000


@pytest.mark.parametrize("case", sorted(MC.SAMPLING) + ["fan"])
def test_surface_area_bitexact(pkg, O, gpu, case):
    V, T = (MC.SAMPLING[case][0] if case in MC.SAMPLING else MC.NORMALS[case])()
    area = _mesh(pkg, V, T).get_surface_area()
    ref = O.surface_area(V, T)
    assert np.float64(area).view(np.uint64) == np.float64(ref).view(np.uint64), f"{case}: {area!r} vs {ref!r}"
    if case == "ties":
        assert ref == 2.0


def _attrs(O, V, T, seed=9):
    rng = np.random.default_rng(seed)
    return O.vertex_normals(V, T), rng.uniform(0, 1, V.shape)


def _check_cloud(pcd, P, PN, PC, what):
    assert_bitwise(np.asarray(pcd.points), P, what + " points")
    if PN is None:
        assert not pcd.has_normals()
    else:
        assert_bitwise(np.asarray(pcd.normals), PN, what + " normals")
    if PC is None:
        assert not pcd.has_colors()
    else:
        assert_bitwise(np.asarray(pcd.colors), PC, what + " colours")


@pytest.mark.parametrize("case", sorted(MC.SAMPLING))
def test_sampling_bitexact(pkg, O, gpu, case):
    """sample_points_uniformly, the fused sample_points_min_z with z_min = -inf (every point kept) and with the median
    z, against the oracle's sampling (+ filter_min_z); seeds 0 and 2^63 + 1; normals and colours both present and both
    absent"""
    build, n_list = MC.SAMPLING[case]
    V, T = build()
    VN, VC = _attrs(O, V, T)
    for attrs in (False, True):
        mesh = _mesh(pkg, V, T, VN if attrs else None, VC if attrs else None)
        for n in n_list:
            for seed in SEEDS:
                what = f"{case}, {n} points, seed {seed}, attributes {attrs}"
                P, PN, PC = O.sample_points_uniformly(V, T, n, seed, VN=VN if attrs else None,
                                                      VC=VC if attrs else None)
                _check_cloud(mesh.sample_points_uniformly(number_of_points=n, seed=seed), P, PN, PC, what)
                _check_cloud(mesh.sample_points_min_z(n, -np.inf, seed=seed), P, None, PC, what + ", fused")
                z_mid = float(np.median(P[:, 2]))
                rx, rc = O.filter_min_z(P, PC, z_mid)
                _check_cloud(mesh.sample_points_min_z(n, z_mid, seed=seed), rx, None, rc, what + ", fused, median z")
    if case == "ties":  # std::round: half away from zero; half to even would put point 0 of N = 2 in triangle 1
        for n, tri in ((2, [0, 2]), (6, [0, 0, 1, 2, 2, 3]), (10, [0, 0, 0, 1, 1, 2, 2, 2, 3, 3])):
            P, _, _ = O.sample_points_uniformly(V, T, n, 0)
            assert np.floor(P[:, 0] / 4.0).astype(int).tolist() == tri
    if case == "zero_area":
        x, y = V[T[:, 0]] - V[T[:, 1]], V[T[:, 0]] - V[T[:, 2]]
        flat = (np.cross(x, y) == 0).all(1)
        assert int(flat.sum()) == MC.ZERO_RUN + 5 and int((~flat).sum()) == 12


def test_sampling_batch_bitexact(pkg, O, gpu):
    """sample_points_uniformly_batch and sample_points_min_z_batch over designed meshes of very different sizes in one
    call: each cloud equals the oracle's for its mesh"""
    names = ["ties", "zero_area", "two_triangles", "skew", "one_triangle", "tiny"]
    built = [MC.SAMPLING[k][0]() for k in names]
    for attrs in (False, True):
        extra = [_attrs(O, V, T) if attrs else (None, None) for V, T in built]
        meshes = [_mesh(pkg, V, T, *e) for (V, T), e in zip(built, extra)]
        for n, seed in ((6, SEEDS[1]), (257, SEEDS[0]), (1000, SEEDS[1])):
            refs = [O.sample_points_uniformly(V, T, n, seed, VN=e[0], VC=e[1]) for (V, T), e in zip(built, extra)]
            clouds = pkg.geometry.TriangleMesh.sample_points_uniformly_batch(meshes, number_of_points=n, seed=seed)
            fused = pkg.geometry.TriangleMesh.sample_points_min_z_batch(meshes, n, 0.0, seed=seed)
            for name, c, f, (P, PN, PC) in zip(names, clouds, fused, refs):
                what = f"batch of {n}, seed {seed}, attributes {attrs}: {name}"
                _check_cloud(c, P, PN, PC, what)
                rx, rc = O.filter_min_z(P, PC, 0.0)
                _check_cloud(f, rx, None, rc, what + ", fused")
