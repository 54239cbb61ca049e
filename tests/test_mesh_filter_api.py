"""The mesh filters without a device (DESIGN.md §4 "mesh filters"): the reference of tests/mesh_filter_ref.py states
every operator as a literal loop and in a vectorised form, and the two agree bit for bit on random soups and on the
designed meshes; known answers; the C ABI declarations and bindings; what the facade raises or returns before any
device work."""
import os
import re

import numpy as np
import pytest

import mesh_component_cases as MC
import mesh_filter_ref as FR
from conftest import ROOT, assert_bitwise

ENTRIES = {
    "ot_mesh_compute_adjacency": 7,
    "ot_mesh_filter": 16,
    "ot_mesh_simplify_vertex_clustering": 15,
}
FILTERS = ((FR.SIMPLE, 0.0, 0.0), (FR.LAPLACIAN, 0.5, 0.0), (FR.TAUBIN, 0.5, -0.53), (FR.SHARPEN, 1.0, 0.0))


def _both_forms(V, T, N, C, what, iterations=(1, 2), scopes=("All",)):
    nv = len(V)
    sets = FR.adjacency_loop(T, nv)
    off, nbr = FR.adjacency_csr(T, nv)
    off2, nbr2 = FR.csr_of_sets(sets)
    assert_bitwise(off, off2, what + ": offsets, loop vs vectorised")
    assert_bitwise(nbr, nbr2, what + ": neighbours, loop vs vectorised")
    for kind, p0, p1 in FILTERS:
        for it in iterations:
            for scope in scopes:
                a = FR.filter_mesh(kind, V, T, N, C, it, p0, p1, scope, loop=True)
                b = FR.filter_mesh(kind, V, T, N, C, it, p0, p1, scope, loop=False)
                for x, y, name in zip(a, b, ("vertices", "normals", "colours")):
                    assert (x is None) == (y is None)
                    if x is not None:
                        assert_bitwise(x, y, f"{what}: {kind} x{it} scope {scope}: {name}, loop vs vectorised")
    for vs in (0.3, 1.1):
        a = FR.simplify_vertex_clustering_loop(V, T, vs, N, C)
        b = FR.simplify_vertex_clustering(V, T, vs, N, C)
        for x, y, name in zip(a, b, ("vertices", "triangles", "normals", "colours")):
            assert (x is None) == (y is None)
            if x is not None:
                assert_bitwise(x, y, f"{what}: clustering at {vs}: {name}, loop vs vectorised")


def test_loop_and_vectorised_forms_agree_on_random_soups():
    soups = MC.random_soups(5, 24)
    for i, tri in enumerate(soups):
        nv = MC.vertex_count(tri) + (i % 3)  # some with trailing isolated vertices
        V = MC.random_vertices(nv, 100 + i)
        N, C = FR.attributes(nv, 200 + i)
        if i % 4 == 3:
            N = C = None
        _both_forms(V, tri, N, C, f"soup {i}")


def test_loop_and_vectorised_forms_agree_on_the_designed_meshes():
    V, T = FR.grid_mesh(9, 9)
    N, C = FR.attributes(len(V), 1)
    _both_forms(V, T, N, C, "grid", iterations=(1, 3), scopes=FR.SCOPES)
    for name, (V, T) in (("isolated", FR.with_isolated_vertices()), ("coincident", FR.coincident_neighbours()),
                         ("self loops", FR.self_loops()), ("tetrahedron", FR.tetrahedron()),
                         ("lattice", FR.unit_lattice(3))):
        N, C = FR.attributes(len(V), 2)
        _both_forms(V, T, N, C, name)
    T = FR.hub_fan(64)
    _both_forms(FR.hub_fan_vertices(64), T, None, None, "hub fan of 64", iterations=(1,))


def test_designed_meshes_are_what_they_claim():
    T = FR.hub_fan(4096)
    off, nbr = FR.adjacency_csr(T, 4097)
    deg = np.diff(off)
    assert deg[0] == 4096 and (deg[1:] == 3).all()
    V, T = FR.with_isolated_vertices()
    deg = np.diff(FR.adjacency_csr(T, len(V))[0])
    assert (deg[:5] == 0).all() and (deg[-65:] == 0).all() and (deg[5:-65] > 0).all()
    V, T = FR.coincident_neighbours()
    sets = FR.adjacency_loop(T, len(V))
    assert 11 in sets[10] and 41 in sets[40] and 49 in sets[40] and 49 in sets[41]
    assert (V[10] == V[11]).all() and (V[40] == V[41]).all() and (V[49] == V[41]).all()
    V, T = FR.self_loops()
    sets = FR.adjacency_loop(T, len(V))
    assert 20 in sets[20] and 33 in sets[33] and 50 in sets[50] and 21 not in sets[21]
    sets = FR.adjacency_loop(MC.degenerate_links(), 13)
    assert sets[5] == {1, 2, 5} and sets[3] == {3} and sets[10] == {10, 11, 12}
    sets = FR.adjacency_loop(MC.duplicate_basics(), 10)
    assert sets[0] == {1, 2} and sets[3] == {3, 7} and sets[5] == {5}  # set semantics: repeats collapse
    with pytest.raises(RuntimeError, match=r"\[ComputeAdjacencyList\] triangle index out of range \[0, n_vertices\)"):
        FR.adjacency_csr(np.array([[0, 1, 3]], np.int32), 3)
    with pytest.raises(RuntimeError, match=r"triangle index out of range"):
        FR.adjacency_loop(np.array([[0, -1, 2]], np.int32), 3)


def test_isolated_vertices_and_zero_lambda_keep_their_bits():
    V, T = FR.with_isolated_vertices()
    N, C = FR.attributes(len(V), 3)
    iso = np.diff(FR.adjacency_csr(T, len(V))[0]) == 0
    for kind, p0, p1 in FILTERS:
        v, n, c = FR.filter_mesh(kind, V, T, N, C, 2, p0, p1)
        for got, want in ((v, V), (n, N), (c, C)):
            assert_bitwise(got[iso], want[iso], f"{kind}: isolated vertices")
            assert not (got[~iso] == want[~iso]).all()
    V, T = FR.grid_mesh(9, 9)
    v, _, _ = FR.filter_mesh(FR.LAPLACIAN, V, T, None, None, 3, 0.0)
    assert_bitwise(v, V, "lambda = 0")  # x + 0 * (finite) = x, and no coordinate of this mesh is -0.0
    v, n, c = FR.filter_mesh(FR.SIMPLE, V, T, V + 1.0, None, 0)
    assert_bitwise(v, V, "no iterations")
    assert c is None
    assert_bitwise(n, V + 1.0, "no iterations: normals")


def test_known_answer_tetrahedron():
    V, T = FR.tetrahedron()
    for loop in (True, False):
        v, _, _ = FR.filter_mesh(FR.SIMPLE, V, T, iterations=1, loop=loop)
        assert_bitwise(v, np.full((4, 3), 3.0), "every vertex lands on the centroid, exactly")
    v, n, c = FR.filter_mesh(FR.SIMPLE, V, T, N=V * 2.0, C=V * 0.5, iterations=1, scope="Normal")
    assert_bitwise(v, V, "scope Normal leaves the vertices")
    assert_bitwise(n, np.full((4, 3), 6.0), "and filters the normals by the same rule, not normalised")
    assert_bitwise(c, V * 0.5, "and leaves the colours")
    v, _, _ = FR.filter_mesh(FR.SHARPEN, V, T, iterations=1, p0=1.0)
    assert_bitwise(v, V * 5.0 - 12.0, "sharpen: x (1 + 3) - (12 - x), exact")


def test_known_answer_unit_lattice():
    V, T = FR.unit_lattice(4)
    for fn in (FR.simplify_vertex_clustering_loop, FR.simplify_vertex_clustering):
        v, t, n, c = fn(V, T, 2.0, N=V * 2.0, C=None)
        # per axis the keys of 0, 1, 2, 3 are 0, 1, 1, 2: 27 voxels with 1, 2 or 1 points per axis
        assert v.shape == (27, 3) and c is None
        axis = {0.0: 1, 1.5: 2, 3.0: 1}
        assert set(np.unique(v).tolist()) == set(axis)
        assert_bitwise(n, v * 2.0, "normals are averaged by the same chain (exact here)")
        # first appearance in x-major order: voxel (i, j, k) is new vertex 9 i + 3 j + k
        centre = np.array([0.0, 1.5, 3.0])
        want = np.stack(np.meshgrid(centre, centre, centre, indexing="ij"), -1).reshape(-1, 3)
        assert_bitwise(v, want, "averages and numbering in closed form")
        assert len(t) and (t[:, 0] < t[:, 1]).all() and (t[:, 0] < t[:, 2]).all()
        assert len(np.unique(t, axis=0)) == len(t)
        assert (t == np.array([0, 9, 3])).all(1).any()  # (v, v + x, v + y) on the coarse lattice


def test_clustering_rules_on_small_cases():
    # four corners far apart, each with a close twin: the quad's triangles collapse onto rotations and a flip
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    V = np.concatenate([base, base + 0.01])
    T = np.array([[0, 1, 2], [5, 6, 4], [2, 4, 1], [0, 6, 1], [6, 7, 4], [0, 4, 1], [3, 7, 3]], np.int32)
    for fn in (FR.simplify_vertex_clustering_loop, FR.simplify_vertex_clustering):
        v, t, _, _ = fn(V, T, 0.25)
        assert_bitwise(v, base + 0.005, "twins average")
        # (0 1 2); its rotation (1 2 0) goes; (2 0 1) goes; the flip (0 2 1) stays; (2 3 0) rotates to (0 2 3);
        # (0 0 1) and (3 3 3) collapse
        assert t.tolist() == [[0, 1, 2], [0, 2, 1], [0, 2, 3]]
    # a permuted vertex order changes the first-appearance numbering
    perm = np.array([7, 2, 5, 0, 3, 6, 1, 4])
    inv = np.argsort(perm)
    v2, t2, _, _ = FR.simplify_vertex_clustering(V[perm], inv[T].astype(np.int32), 0.25)
    assert_bitwise(v2, (base + 0.005)[[3, 2, 1, 0]], "numbered by first appearance")
    with pytest.raises(RuntimeError, match=r"\[SimplifyVertexClustering\] voxel_size <= 0\."):
        FR.simplify_vertex_clustering(V, T, 0.0)
    with pytest.raises(RuntimeError, match=r"\[SimplifyVertexClustering\] voxel_size is too small\."):
        FR.simplify_vertex_clustering(V * 1e6, T, 1e-4)


# ------------------------------------------------------------------------------------------------ the interface
def test_header_declares_and_table_binds_the_entries(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.native_library()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bot_status\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(pkg._lib.SIGNATURES[name]) == nargs, name
        assert name not in lib._ot_missing
    assert lib.ot_abi_version() == 1


def test_facade_has_the_methods_and_enums(pkg):
    G = pkg.geometry
    for name in ("compute_adjacency_list", "has_adjacency_list", "filter_smooth_simple", "filter_smooth_laplacian",
                 "filter_smooth_taubin", "filter_sharpen", "simplify_vertex_clustering"):
        assert callable(getattr(G.TriangleMesh, name)), name
    assert isinstance(G.TriangleMesh.adjacency_list, property)
    assert [m.name for m in G.FilterScope] == ["All", "Color", "Normal", "Vertex"]
    assert [m.name for m in G.SimplificationContraction] == ["Average", "Quadric"]
    mesh = G.TriangleMesh()
    assert not mesh.has_adjacency_list() and mesh.adjacency_list == []


def _no_native_calls(pkg, monkeypatch):
    def refuse(name, *args):
        raise AssertionError(f"native call {name} where none is expected")
    monkeypatch.setattr(pkg._lib, "call", refuse)


def test_refusals_come_before_any_device_work(pkg, monkeypatch):
    G = pkg.geometry
    _no_native_calls(pkg, monkeypatch)
    V, T = FR.tetrahedron()
    mesh = G.TriangleMesh(V, T)
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match=r"\[SimplifyVertexClustering\] voxel_size <= 0\."):
            mesh.simplify_vertex_clustering(vs)
    with pytest.raises(RuntimeError, match=r"SimplificationContraction\.Quadric is not supported by this build"):
        mesh.simplify_vertex_clustering(0.5, G.SimplificationContraction.Quadric)
    with pytest.raises(RuntimeError, match=r"Quadric"):
        mesh.simplify_vertex_clustering(0.5, contraction=G.SimplificationContraction.Quadric)
    assert_bitwise(np.asarray(mesh.vertices), V, "a refused call leaves the mesh alone")


def test_c_abi_refusals_need_no_device(pkg):
    import ctypes as C

    lib = pkg.native_library()
    bad = pkg._lib.OT_ERR_INVALID_ARGUMENT
    k, k2 = C.c_int64(7), C.c_int64(7)
    buf = np.zeros((8, 3))
    ibuf = np.zeros((8, 3), np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    ip = ibuf.ctypes.data_as(C.c_void_p)
    assert lib.ot_mesh_simplify_vertex_clustering(p, None, None, 4, ip, 2, 0.0, 0, p, None, None, C.byref(k), ip,
                                                  C.byref(k2), None) == bad
    assert lib.ot_last_error().decode() == "[SimplifyVertexClustering] voxel_size <= 0."
    assert lib.ot_mesh_simplify_vertex_clustering(p, None, None, 4, ip, 2, 0.5, 1, p, None, None, C.byref(k), ip,
                                                  C.byref(k2), None) == bad
    assert "Quadric is not supported by this build" in lib.ot_last_error().decode()
    assert lib.ot_mesh_simplify_vertex_clustering(None, None, None, 0, None, 0, 0.5, 0, None, None, None, C.byref(k),
                                                  None, C.byref(k2), None) == 0
    assert k.value == 0 and k2.value == 0
    assert lib.ot_mesh_compute_adjacency(ip, 2, 4, None, ip, C.byref(k), None) == bad
    assert lib.ot_last_error().decode().startswith("[ComputeAdjacencyList]")
    assert lib.ot_mesh_compute_adjacency(ip, 2 ** 31 // 6 + 1, 4, ip, ip, C.byref(k), None) == bad
    assert lib.ot_mesh_compute_adjacency(ip, -1, 4, ip, ip, C.byref(k), None) == bad
    assert lib.ot_mesh_filter(9, p, None, None, 4, ip, ip, 0, 1, 0.5, 0.0, 7, p, None, None, None) == bad
    assert lib.ot_mesh_filter(0, p, None, None, 4, ip, ip, 0, 1, 0.5, 0.0, 7, p, None, None, None) == bad  # aliases
    assert lib.ot_last_error().decode().startswith("[FilterMesh]")
    assert lib.ot_mesh_filter(0, None, None, None, 0, None, None, 0, 1, 0.5, 0.0, 7, None, None, None, None) == 0


def test_copies_without_a_native_call(pkg, monkeypatch):
    G, U = pkg.geometry, pkg.utility
    _no_native_calls(pkg, monkeypatch)
    V, T = FR.tetrahedron()
    mesh = G.TriangleMesh(V, T)
    mesh.vertex_normals = U.Vector3dVector(V + 1.0)
    mesh.vertex_colors = U.Vector3dVector(V * 0.125)
    calls = (lambda m, n: m.filter_smooth_simple(n), lambda m, n: m.filter_smooth_laplacian(n, 0.5),
             lambda m, n: m.filter_smooth_taubin(n, 0.5, -0.53), lambda m, n: m.filter_sharpen(n, 1.0),
             lambda m, n: m.filter_smooth_simple(number_of_iterations=n, scope=G.FilterScope.Vertex))
    for call in calls:
        for n in (0, -3):
            out = call(mesh, n)
            assert out is not mesh
            assert_bitwise(np.asarray(out.vertices), V, "the copy's vertices")
            assert_bitwise(np.asarray(out.triangles), T, "the copy's triangles")
            assert_bitwise(np.asarray(out.vertex_normals), V + 1.0, "the copy's normals")
            assert_bitwise(np.asarray(out.vertex_colors), V * 0.125, "the copy's colours")
            np.asarray(out.vertices)[0, 0] = 99.0  # a copy: the input does not see it
            assert np.asarray(mesh.vertices)[0, 0] == V[0, 0]
    empty = G.TriangleMesh()
    for call in calls:
        out = call(empty, 2)
        assert out is not empty and len(out.vertices) == 0 and len(out.triangles) == 0
    out = empty.simplify_vertex_clustering(0.5)
    assert out is not empty and len(out.vertices) == 0 and len(out.triangles) == 0
    assert empty.compute_adjacency_list() is empty and not empty.has_adjacency_list()


def test_assignments_drop_the_adjacency_list(pkg):
    G, U = pkg.geometry, pkg.utility
    V, T = FR.tetrahedron()
    csr = FR.adjacency_csr(T, 4)
    drops = (lambda m: setattr(m, "triangles", U.Vector3iVector(T)), lambda m: setattr(m, "vertices", U.Vector3dVector(V)),
             lambda m: m.remove_triangles_by_index([]) if len(m.triangles) == 0 else None)
    for drop, tri in zip(drops, (T, T, None)):
        mesh = G.TriangleMesh(V, tri)
        # as compute_adjacency_list leaves it (host arrays stand in for the device's)
        mesh._adj = csr if tri is not None else (np.zeros(5, np.int32), np.zeros(0, np.int32))
        assert mesh.has_adjacency_list()
        assert mesh.adjacency_list == ([{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}] if tri is not None else [set()] * 4)
        drop(mesh)
        assert not mesh.has_adjacency_list() and mesh.adjacency_list == []
