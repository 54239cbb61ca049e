"""GPU parity of TriangleMesh.compute_adjacency_list, filter_smooth_simple / _laplacian / _taubin, filter_sharpen and
simplify_vertex_clustering (csrc/mesh_filter.hip) against the numpy restatement of tests/mesh_filter_ref.py (its
vectorised forms, which test_mesh_filter_api.py ties to the literal loops on the CPU).  Positions, normals, colours,
triangles, offsets and neighbours are compared bit for bit: both sides perform the same float64 operations in the same
order, and float64 sqrt and division are correctly rounded on both, so there is no tolerance."""
import numpy as np
import pytest

import mc_volumes as MV
import mesh_component_cases as MC
import mesh_filter_ref as FR
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

KINDS = {
    FR.SIMPLE: (0.0, 0.0, lambda m, it, p0, p1, s: m.filter_smooth_simple(it, scope=s)),
    FR.LAPLACIAN: (0.5, 0.0, lambda m, it, p0, p1, s: m.filter_smooth_laplacian(it, p0, scope=s)),
    FR.TAUBIN: (0.5, -0.53, lambda m, it, p0, p1, s: m.filter_smooth_taubin(it, p0, p1, scope=s)),
    FR.SHARPEN: (0.7, 0.0, lambda m, it, p0, p1, s: m.filter_sharpen(it, p0, scope=s)),
}


def _mesh(pkg, V, T, N=None, C=None):
    m = pkg.geometry.TriangleMesh(V, T)
    if N is not None:
        m.vertex_normals = pkg.utility.Vector3dVector(N)
    if C is not None:
        m.vertex_colors = pkg.utility.Vector3dVector(C)
    return m


def _tri(mesh):
    return np.asarray(mesh.triangles, np.int32).reshape(-1, 3)


def _same_mesh(mesh, V, T, N, C, what):
    assert_bitwise(np.asarray(mesh.vertices), V, what + ": vertices")
    assert_bitwise(_tri(mesh), T, what + ": triangles")
    assert mesh.has_vertex_normals() == (N is not None) and mesh.has_vertex_colors() == (C is not None), what
    if N is not None:
        assert_bitwise(np.asarray(mesh.vertex_normals), N, what + ": normals")
    if C is not None:
        assert_bitwise(np.asarray(mesh.vertex_colors), C, what + ": colours")


def _check_filter(pkg, V, T, N, C, kind, it, scope, what, mesh=None):
    p0, p1, call = KINDS[kind]
    what = f"{what}: {kind} x{it} scope {scope}"
    mesh = mesh if mesh is not None else _mesh(pkg, V, T, N, C)
    out = call(mesh, it, p0, p1, getattr(pkg.geometry.FilterScope, scope))
    assert out is not mesh
    rv, rn, rc = FR.filter_mesh(kind, V, T, N, C, it, p0, p1, scope)
    _same_mesh(out, rv, T, rn, rc, what)
    _same_mesh(mesh, V, T, N, C, what + ": the input is untouched")
    assert out.has_adjacency_list()
    return out


@pytest.fixture(scope="module")
def noise_mesh(pkg, gpu):
    """the marching-cubes mesh of mc_volumes.noise() through the package's own extraction, with vertex normals:
    (V, T, N, C) on the host"""
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = MV.noise()
    vol = integ.ScalableTSDFVolume(voxel_length=MV.VOXEL_LENGTH, sdf_trunc=0.04,
                                   color_type=integ.TSDFVolumeColorType.RGB8, color_precision=64, max_units=64)
    vol.import_units(keys, tsdf, weight, color)
    mesh = vol.extract_triangle_mesh()
    mesh.compute_vertex_normals()
    V, T, N, C = (np.array(a) for a in (mesh.vertices, mesh.triangles, mesh.vertex_normals, mesh.vertex_colors))
    assert len(V) > 1000 and len(N) == len(V) == len(C)
    return V, np.ascontiguousarray(T.astype(np.int32)), N, C


# ---------------------------------------------------------------------------------------------------- adjacency
def _check_adjacency(pkg, T, nv, what):
    mesh = _mesh(pkg, MC.random_vertices(nv, 5), T)
    assert not mesh.has_adjacency_list()
    assert mesh.compute_adjacency_list() is mesh
    assert mesh.has_adjacency_list()
    off, nbr = FR.adjacency_csr(T, nv)
    got_off, got_nbr = (t.cpu().numpy() for t in mesh._adj)
    assert got_off.dtype == got_nbr.dtype == np.int32
    assert_bitwise(got_off, off, what + ": offsets")
    assert_bitwise(got_nbr, nbr, what + ": neighbours")
    sets = mesh.adjacency_list
    assert isinstance(sets, list) and len(sets) == nv and all(isinstance(s, set) for s in sets)
    assert all(type(x) is int for s in sets[:8] for x in s)
    if len(T) <= 700:
        assert sets == FR.adjacency_loop(T, nv), what
    assert_bitwise(_tri(mesh), T, what + ": the triangles are left alone")
    return mesh, sets


def test_adjacency_designed_meshes(pkg, gpu):
    _, sets = _check_adjacency(pkg, MC.bow_tie(), 5, "bow-tie")
    assert sets[2] == {0, 1, 3, 4}
    _, sets = _check_adjacency(pkg, MC.bow_tie_fan(100), 201, "fan of 100 bow-ties")
    assert len(sets[0]) == 200
    _, sets = _check_adjacency(pkg, MC.degenerate_links(), 13, "degenerate links")
    assert sets[5] == {1, 2, 5} and sets[3] == {3} and sets[0] == set()  # self-loops kept, vertex 0 unreferenced
    _, sets = _check_adjacency(pkg, MC.duplicate_basics(), 10, "duplicates")
    assert sets[0] == {1, 2} and sets[3] == {3, 7}  # set semantics
    for n in MC.SIZES:
        _check_adjacency(pkg, MC.isolated(n), 3 * n + 2, f"{n} isolated triangles")
    two = MC.two_strips(2048)
    _check_adjacency(pkg, two, MC.vertex_count(two), "two interleaved strips")
    _, sets = _check_adjacency(pkg, FR.hub_fan(4096), 4097, "hub fan")
    assert len(sets[0]) == 4096 and all(len(s) == 3 for s in sets[1:])
    _, sets = _check_adjacency(pkg, np.array([[2, 0, 1]], np.int32), 3, "one triangle")
    assert sets == [{1, 2}, {0, 2}, {0, 1}]
    mesh, sets = _check_adjacency(pkg, np.zeros((0, 3), np.int32), 4, "no triangles")
    assert sets == [set()] * 4


def test_adjacency_random_soups(pkg, gpu):
    for i, tri in enumerate(MC.random_soups(7, 20)):
        _check_adjacency(pkg, tri, MC.vertex_count(tri) + i % 2, f"soup {i}")


@pytest.mark.parametrize("bad", ["n_vertices", -1])
def test_adjacency_out_of_range_index_is_refused(pkg, gpu, bad):
    good = MC.nonmanifold_runs()
    nv = MC.vertex_count(good)
    tri = good.copy()
    tri[len(tri) // 2, 1] = nv if bad == "n_vertices" else -1
    V = MC.random_vertices(nv, 1)
    mesh = _mesh(pkg, V, tri)
    with pytest.raises(RuntimeError) as e:
        mesh.compute_adjacency_list()
    assert str(e.value) == "[ComputeAdjacencyList] triangle index out of range [0, n_vertices)"
    assert not mesh.has_adjacency_list()
    _same_mesh(mesh, V, tri, None, None, "a refused call leaves the mesh alone")
    for call in (lambda: mesh.filter_smooth_simple(1), lambda: mesh.filter_smooth_taubin(2)):
        with pytest.raises(RuntimeError, match=r"\[ComputeAdjacencyList\] triangle index out of range"):
            call()
    with pytest.raises(RuntimeError) as e:
        mesh.simplify_vertex_clustering(0.1)
    assert str(e.value) == "[SimplifyVertexClustering] triangle index out of range [0, n_vertices)"
    _same_mesh(mesh, V, tri, None, None, "after the refusals")
    _check_adjacency(pkg, good, nv, "the next valid call")


def test_adjacency_is_dropped_and_rebuilt(pkg, gpu):
    V, T = FR.grid_mesh(9, 9)
    mesh = _mesh(pkg, V, T).compute_adjacency_list()
    mesh.remove_triangles_by_index([0, 1, 2])
    assert not mesh.has_adjacency_list()
    T2 = np.delete(T, [0, 1, 2], axis=0)
    out = mesh.filter_smooth_simple(1)  # built again, on the copy
    assert_bitwise(np.asarray(out.vertices), FR.filter_mesh(FR.SIMPLE, V, T2)[0], "filtered on the new triangles")
    assert not mesh.has_adjacency_list() and out.has_adjacency_list()
    mesh.compute_adjacency_list()
    for call in (mesh.remove_degenerate_triangles, mesh.remove_duplicated_triangles, mesh.remove_unreferenced_vertices):
        mesh.compute_adjacency_list()
        call()
        assert not mesh.has_adjacency_list()


# ------------------------------------------------------------------------------------------------------ filters
def _filter_cases():
    V, T = FR.grid_mesh(33, 33)
    N, C = FR.attributes(len(V), 1)
    yield "grid 33 x 33", V, T, N, C
    yield "grid 33 x 33, no normals or colours", V, T, None, None
    Vh = FR.hub_fan_vertices(4096)
    Nh, Ch = FR.attributes(len(Vh), 2)
    yield "hub fan", Vh, FR.hub_fan(4096), Nh, Ch
    Vi, Ti = FR.with_isolated_vertices()
    Ni, Ci = FR.attributes(len(Vi), 3)
    yield "isolated vertices", Vi, Ti, Ni, Ci
    Vc, Tc = FR.coincident_neighbours()
    Nc, Cc = FR.attributes(len(Vc), 4)
    yield "coincident neighbours", Vc, Tc, Nc, Cc
    Vs, Ts = FR.self_loops()
    Ns, Cs = FR.attributes(len(Vs), 5)
    yield "self loops", Vs, Ts, Ns, None


FILTER_CASES = {c[0]: c[1:] for c in _filter_cases()}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", list(FILTER_CASES))
def test_filters_designed_meshes(pkg, gpu, case, kind):
    V, T, N, C = FILTER_CASES[case]
    small = len(V) < 2000
    for it in (1, 2, 5):
        for scope in (FR.SCOPES if (small or it == 2) else ("All",)):
            _check_filter(pkg, V, T, N, C, kind, it, scope, case)


def test_filters_keep_isolated_vertices(pkg, gpu):
    V, T, N, C = FILTER_CASES["isolated vertices"]
    iso = np.diff(FR.adjacency_csr(T, len(V))[0]) == 0
    assert iso.sum() == 70
    for kind in KINDS:
        out = _check_filter(pkg, V, T, N, C, kind, 3, "All", "isolated")
        for got, want in ((out.vertices, V), (out.vertex_normals, N), (out.vertex_colors, C)):
            assert_bitwise(np.asarray(got)[iso], want[iso], f"{kind}: isolated vertices keep their bits")
            assert np.isfinite(np.asarray(got)).all()
    lone = _mesh(pkg, V, np.zeros((0, 3), np.int32), N, C)  # no triangles at all: every vertex is isolated
    _same_mesh(lone.filter_smooth_laplacian(2), V, np.zeros((0, 3), np.int32), N, C, "a mesh without triangles")


def test_filters_coincident_neighbours_weight(pkg, gpu):
    V, T, N, C = FILTER_CASES["coincident neighbours"]
    out = _check_filter(pkg, V, T, N, C, FR.LAPLACIAN, 1, "All", "coincident")
    got = np.asarray(out.vertices)
    assert np.isfinite(got).all()
    # weight 1e12 against weights of about 1 / 0.05: vertex 10 all but stays on its twin
    assert np.abs(got[10] - (V[10] + 0.5 * (V[11] - V[10]))).max() < 1e-9


def test_filters_extracted_mesh(pkg, gpu, noise_mesh):
    V, T, N, C = noise_mesh
    print(f"noise mesh: {len(V)} vertices, {len(T)} triangles")
    mesh = _mesh(pkg, V, T, N, C).compute_adjacency_list()
    for kind in KINDS:
        for it in (1, 2, 5):
            _check_filter(pkg, V, T, N, C, kind, it, "All", "extracted mesh", mesh=mesh)
    for scope in FR.SCOPES:
        _check_filter(pkg, V, T, N, C, FR.TAUBIN, 2, scope, "extracted mesh", mesh=mesh)


def test_taubin_is_alternating_laplacian_steps(pkg, gpu):
    V, T, N, C = FILTER_CASES["grid 33 x 33"]
    lam, mu = 0.5, -0.53
    v, n, c = V, N, C
    for _ in range(3):
        v, n, c = FR.filter_mesh(FR.LAPLACIAN, v, T, n, c, 1, lam)
        v, n, c = FR.filter_mesh(FR.LAPLACIAN, v, T, n, c, 1, mu)
    out = _mesh(pkg, V, T, N, C).filter_smooth_taubin(3, lam, mu)
    _same_mesh(out, v, T, n, c, "Taubin x3 = (lambda, mu) x3 in the reference")
    step = _mesh(pkg, V, T, N, C)
    for _ in range(3):
        step = step.filter_smooth_laplacian(1, lam).filter_smooth_laplacian(1, mu)
    _same_mesh(step, v, T, n, c, "and = six single Laplacian calls on the GPU")


def test_zero_lambda_defaults_and_repeatability(pkg, gpu):
    V, T, N, C = FILTER_CASES["grid 33 x 33"]
    mesh = _mesh(pkg, V, T, N, C)
    _same_mesh(mesh.filter_smooth_laplacian(3, 0.0), V, T, N, C, "lambda_filter = 0 returns the input bits")
    _same_mesh(mesh.filter_smooth_simple(0), V, T, N, C, "no iterations")
    d = mesh.filter_smooth_taubin()
    rv, rn, rc = FR.filter_mesh(FR.TAUBIN, V, T, N, C, 1, 0.5, -0.53)
    _same_mesh(d, rv, T, rn, rc, "Taubin defaults: one iteration, 0.5, -0.53, scope All")
    _same_mesh(mesh.filter_sharpen(), *(lambda r: (r[0], T, r[1], r[2]))(FR.filter_mesh(FR.SHARPEN, V, T, N, C, 1, 1.0)),
               "sharpen defaults: one iteration, strength 1")
    for kind in KINDS:
        p0, p1, call = KINDS[kind]
        a = call(mesh, 5, p0, p1, pkg.geometry.FilterScope.All)
        b = call(mesh, 5, p0, p1, pkg.geometry.FilterScope.All)
        _same_mesh(b, np.asarray(a.vertices), T, np.asarray(a.vertex_normals), np.asarray(a.vertex_colors),
                   f"{kind}: two calls give the same bits")
    _same_mesh(mesh, V, T, N, C, "the input after all of it")


# --------------------------------------------------------------------------------------------------- clustering
def _check_clustering(pkg, V, T, vs, what, N=None, C=None):
    mesh = _mesh(pkg, V, T, N, C)
    out = mesh.simplify_vertex_clustering(vs)
    assert out is not mesh
    rv, rt, rn, rc = FR.simplify_vertex_clustering(V, T, vs, N, C)
    _same_mesh(out, rv, rt, rn, rc, f"{what} at {vs}")
    _same_mesh(mesh, V, T, N, C, what + ": the input is untouched")
    assert out._mc is None and not out.has_adjacency_list()
    return out, rv, rt


def _random_triangles(nv, nt, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, nv, (nt, 3)).astype(np.int32))


def test_clustering_vertices_on_voxel_faces(pkg, gpu):
    g = np.arange(-8, 9) * 0.125  # -1 .. 1: min - vs / 2 + k vs = -1.125 + 0.25 k hits every odd multiple of 0.125
    V = np.stack(np.meshgrid(g, g, g[:5], indexing="ij"), -1).reshape(-1, 3)
    V = V[np.random.default_rng(3).permutation(len(V))]
    T = _random_triangles(len(V), 3000, 4)
    N, C = FR.attributes(len(V), 6)
    on_face = ((V[:, 0] + 1.125) / 0.25 == np.floor((V[:, 0] + 1.125) / 0.25))
    assert 0 < on_face.sum() < len(V)
    _check_clustering(pkg, V, T, 0.25, "vertices on voxel faces, negative coordinates", N, C)
    far = np.array([1024.0, -2048.0, 512.0])
    _check_clustering(pkg, V + far, T, 0.25, "the same at a far offset", N, C)
    _check_clustering(pkg, V + far, T, 0.3, "and with a voxel size that is not representable", N, C)


def test_clustering_one_voxel_and_long_chains(pkg, gpu):
    rng = np.random.default_rng(8)
    V = rng.uniform(0.0, 1.0, (500, 3))
    out, _, _ = _check_clustering(pkg, V, _random_triangles(500, 900, 9), 10.0, "everything in one voxel")
    assert len(out.vertices) == 1 and len(out.triangles) == 0
    # 4 096 vertices in one voxel, spread over magnitudes so that the order of the chain shows, beside singletons
    # (the first voxel is [min - 0.5, min + 0.5) per axis with min in [0, 4e-7): the blob stays below 0.4)
    blob = rng.uniform(0.0, 0.4, (4096, 3)) * 10.0 ** rng.integers(-6, 1, (4096, 1))
    singles = np.stack([np.arange(2, 302) * 1.0 + 0.5, np.zeros(300), np.zeros(300)], 1)
    V = np.concatenate([blob, singles])[rng.permutation(4396)]
    assert np.bincount(np.unique(FR.voxel_keys(V, 1.0), axis=0, return_inverse=True)[1].reshape(-1)).max() == 4096
    N, C = FR.attributes(len(V), 10)
    out, rv, _ = _check_clustering(pkg, V, _random_triangles(len(V), 4000, 11), 1.0, "4 096 in one voxel", N, C)
    assert len(rv) == 301
    _check_clustering(pkg, V, np.zeros((0, 3), np.int32), 1.0, "vertices and no triangles", N, C)


def test_clustering_rotations_flips_and_numbering(pkg, gpu):
    V, T = FR.unit_lattice(6)
    rng = np.random.default_rng(12)
    pick = T[rng.integers(0, len(T), 200)]
    rot = np.stack([np.roll(p, int(r)) for p, r in zip(pick, rng.integers(0, 3, 200))])
    flips = pick[:60, ::-1]
    T2 = np.ascontiguousarray(np.concatenate([T, rot, flips, T[:10, [0, 0, 1]]])[rng.permutation(len(T) + 270)])
    out, rv, rt = _check_clustering(pkg, V, T2, 0.5, "every vertex in its own voxel")
    assert_bitwise(rv, V, "the vertices come back as they were")
    assert len(rt) < len(T2) and (rt[:, 0] < rt[:, 1]).all() and (rt[:, 0] < rt[:, 2]).all()
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    Vq = np.concatenate([base, base + 0.01])
    Tq = np.array([[0, 1, 2], [5, 6, 4], [2, 4, 1], [0, 6, 1], [6, 7, 4], [0, 4, 1], [3, 7, 3]], np.int32)
    out, _, rt = _check_clustering(pkg, Vq, Tq, 0.25, "rotations collapse, flips stay")
    assert rt.tolist() == [[0, 1, 2], [0, 2, 1], [0, 2, 3]]
    perm = np.array([7, 2, 5, 0, 3, 6, 1, 4])
    out, rv, _ = _check_clustering(pkg, Vq[perm], np.argsort(perm)[Tq].astype(np.int32), 0.25, "permuted vertex order")
    assert_bitwise(rv, (base + 0.005)[[3, 2, 1, 0]], "numbered by first appearance")
    Vg, Tg = FR.grid_mesh(33, 33)
    p = rng.permutation(len(Vg))
    a, _, _ = _check_clustering(pkg, Vg, Tg, 0.12, "grid")
    b, _, _ = _check_clustering(pkg, Vg[p], np.argsort(p)[Tg].astype(np.int32), 0.12, "grid, permuted")
    assert len(a.vertices) == len(b.vertices) and not (np.asarray(a.vertices) == np.asarray(b.vertices)).all()


def test_clustering_extracted_meshes(pkg, gpu, noise_mesh):
    V, T, N, C = noise_mesh
    out, rv, rt = _check_clustering(pkg, V, T, 2.5 * MV.VOXEL_LENGTH, "noise mesh", N, C)
    print(f"noise mesh: {len(V)} -> {len(rv)} vertices, {len(T)} -> {len(rt)} triangles")
    assert 0 < len(rv) < len(V) and 0 < len(rt) < len(T)
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = MC.two_spheres()
    vol = integ.ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8,
                                   color_precision=64, max_units=64)
    vol.import_units(keys, tsdf, weight, color)
    mesh = vol.extract_triangle_mesh()
    Vs, Ts, Cs = np.array(mesh.vertices), np.array(mesh.triangles).astype(np.int32), np.array(mesh.vertex_colors)
    out = mesh.simplify_vertex_clustering(0.03)  # straight from the extraction, arrays still on the device
    rv, rt, _, rc = FR.simplify_vertex_clustering(Vs, Ts, 0.03, None, Cs)
    _same_mesh(out, rv, rt, None, rc, "two spheres")
    assert len(out.cluster_connected_triangles()[1]) >= 2


def test_clustering_refusals(pkg, gpu):
    V, T = FR.grid_mesh(9, 9)
    mesh = _mesh(pkg, V, T)
    with pytest.raises(RuntimeError) as e:
        mesh.simplify_vertex_clustering(0.0)
    assert str(e.value) == "[SimplifyVertexClustering] voxel_size <= 0."
    big = _mesh(pkg, V * 1e6, T)
    with pytest.raises(RuntimeError) as e:
        big.simplify_vertex_clustering(1e-4)
    assert str(e.value) == "[SimplifyVertexClustering] voxel_size is too small."
    with pytest.raises(RuntimeError, match=r"voxel_size is too small"):
        FR.simplify_vertex_clustering(V * 1e6, T, 1e-4)
    with pytest.raises(RuntimeError, match=r"Quadric is not supported by this build"):
        mesh.simplify_vertex_clustering(0.1, pkg.geometry.SimplificationContraction.Quadric)
    _same_mesh(big, V * 1e6, T, None, None, "a refused call leaves the mesh alone")
    _check_clustering(pkg, V, T, 0.1, "the next valid call")


# ----------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_smooth_simplify_normals_sample(pkg, gpu, O, noise_mesh):
    """extract -> filter_smooth_taubin(10) -> simplify_vertex_clustering -> compute_vertex_normals ->
    sample_points_uniformly, against the same chain in the references, stage by stage"""
    V, T, N, C = noise_mesh
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = MV.noise()
    vol = integ.ScalableTSDFVolume(voxel_length=MV.VOXEL_LENGTH, sdf_trunc=0.04,
                                   color_type=integ.TSDFVolumeColorType.RGB8, color_precision=64, max_units=64)
    vol.import_units(keys, tsdf, weight, color)
    mesh = vol.extract_triangle_mesh()
    mesh.compute_vertex_normals()  # deferred on a side stream: the filter waits for it
    smooth = mesh.filter_smooth_taubin(10)
    v1, n1, c1 = FR.filter_mesh(FR.TAUBIN, V, T, N, C, 10, 0.5, -0.53)
    _same_mesh(smooth, v1, T, n1, c1, "pipeline: Taubin x10")
    assert smooth._mc is None
    small = smooth.simplify_vertex_clustering(2.0 * MV.VOXEL_LENGTH)
    v2, t2, n2, c2 = FR.simplify_vertex_clustering(v1, T, 2.0 * MV.VOXEL_LENGTH, n1, c1)
    _same_mesh(small, v2, t2, n2, c2, "pipeline: clustering")
    assert small.compute_vertex_normals() is small  # the generic path: these arrays are no extraction's
    n3 = O.vertex_normals(v2, t2)
    assert_bitwise(np.asarray(small.vertex_normals), n3, "pipeline: vertex normals")
    pcd = small.sample_points_uniformly(5000, seed=7)
    P, PN, PC = O.sample_points_uniformly(v2, t2, 5000, 7, VN=n3, VC=c2)
    assert_bitwise(np.asarray(pcd.points), P, "pipeline: sampled points")
    assert_bitwise(np.asarray(pcd.normals), PN, "pipeline: sampled normals")
    assert_bitwise(np.asarray(pcd.colors), PC, "pipeline: sampled colours")
