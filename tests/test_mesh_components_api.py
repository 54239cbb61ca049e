"""TriangleMesh.cluster_connected_triangles and the triangle clean-up calls without a device: the reference
(tests/mesh_components_ref.py) states Open3D's loop and the closed form the GPU computes, and they agree on random
triangle soups, their permutations and every designed mesh of tests/mesh_component_cases.py, whose properties are
asserted here; the C ABI declarations and bindings; the errors that are raised before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_component_cases as MC
import mesh_components_ref as MR
from conftest import ROOT, assert_bitwise

ENTRIES = {
    "ot_mesh_cluster_connected_triangles": 9,
    "ot_mesh_flag_degenerate_triangles": 5,
    "ot_mesh_flag_duplicated_triangles": 5,
    "ot_mesh_remove_triangles_by_mask": 6,
    "ot_mesh_remove_unreferenced_vertices": 6,
}


def _agree(tri, what):
    loop, loop_n = MR.cluster_loop(tri)
    closed, closed_n = MR.cluster_closed(tri)
    assert loop.dtype == closed.dtype == np.int32
    assert_bitwise(loop, closed, f"{what}: Open3D's loop vs the closed form")
    assert list(loop_n) == list(closed_n), what
    assert sum(closed_n) == len(tri)
    return closed, closed_n


def _nonmanifold(tri):
    _, runs = MR.sorted_edge_positions(tri)
    return any(e - s > 2 for s, e in runs.values())


def test_loop_and_closed_form_agree_on_random_soups():
    soups = MC.random_soups(3)
    assert len(soups) >= 50
    multi = nonmanifold = degenerate = duplicated = 0
    for i, tri in enumerate(soups):
        assert 1 <= len(tri) <= 500
        lab, sizes = _agree(tri, f"soup {i}")
        multi += int(len(sizes) >= 2)
        nonmanifold += int(_nonmanifold(tri))
        degenerate += int(MR.degenerate_mask(tri).any())
        duplicated += int(MR.duplicated_mask(tri).any())
        perm = np.random.default_rng(i).permutation(len(tri))
        _agree(tri[perm], f"soup {i} permuted")
    assert multi > 10 and nonmanifold > 10 and degenerate > 10 and duplicated > 10  # the sweep holds every kind


def test_bow_ties_and_edge_direction():
    lab, sizes = _agree(MC.bow_tie(), "bow-tie")
    assert lab.tolist() == [0, 1] and sizes == [1, 1]
    fan = MC.bow_tie_fan(100)
    lab, sizes = _agree(fan, "fan of 100 bow-ties")
    assert lab.tolist() == list(range(100))
    assert (fan[:, 0] == 0).all() and len(np.unique(fan[:, 1:])) == 200  # one shared vertex, no shared edge
    lab, _ = _agree(MC.opposite_edges(), "opposite and equal edge directions")
    assert lab.tolist() == [0, 0, 1, 1, 2]


def test_nonmanifold_runs_cross_the_block_boundaries():
    for k in (5, 300):
        lab, sizes = _agree(MC.shared_edge(k), f"one edge shared by {k}")
        assert sizes == [k]
    tri = MC.nonmanifold_runs()
    assert len(tri) <= 5000
    lab, sizes = _agree(tri, "two runs of 300 on one edge each")
    assert sizes == [1] * MC.NM_FILL + [MC.NM_RUN, MC.NM_RUN]
    _, runs = MR.sorted_edge_positions(tri)
    (s0, e0), (s1, e1) = runs[MC.NM_EDGES[0]], runs[MC.NM_EDGES[1]]
    assert e0 - s0 == e1 - s1 == MC.NM_RUN
    assert s0 < 256 < e0 - 1 and s1 < 1024 < e1 - 1  # the runs of equal keys really straddle 256 and 1024
    rng = np.random.default_rng(29)
    _agree(tri[rng.permutation(len(tri))], "the same, permuted")


def test_degenerate_triangles_link_through_their_own_key():
    tri = MC.degenerate_links()
    lab, _ = _agree(tri, "degenerate links")
    assert lab.tolist() == MC.DEGENERATE_LINK_LABELS
    assert MR.edge_keys(tri)[3].tolist() == [[5, 5]] * 3


def test_strips_are_one_cluster():
    s = MC.strip(4096)
    rng = np.random.default_rng(31)
    for name, t in (("index order", s), ("reversed", s[::-1]), ("permuted", s[rng.permutation(len(s))])):
        lab, sizes = _agree(t, f"strip of 4096, {name}")
        assert sizes == [4096] and (lab == 0).all()
    _, runs = MR.sorted_edge_positions(s)
    assert max(e - b for b, e in runs.values()) == 2  # only consecutive triangles share an edge
    two = MC.two_strips()
    assert len(two) <= 5000
    lab, sizes = _agree(two, "two interleaved strips")
    assert sizes == [2048, 2048] and (lab[0::2] == 0).all() and (lab[1::2] == 1).all()


def test_numbering_is_by_smallest_triangle_index():
    tri = MC.numbering()
    lab, _ = _agree(tri, "numbering")
    assert lab.tolist() == [0, 0, 1, 1]
    by_vertex = [int(tri[lab == k].min()) for k in (0, 1)]
    assert by_vertex[1] < by_vertex[0]  # numbering by smallest vertex index would swap the two


def test_isolated_sizes_and_big_indices():
    for n in MC.SIZES:
        lab, sizes = _agree(MC.isolated(n), f"{n} isolated triangles")
        assert lab.tolist() == list(range(n)) and sizes == [1] * n
    lab, sizes = _agree(np.zeros((0, 3), np.int32), "no triangles")
    assert len(lab) == 0 and sizes == []
    tri = MC.big_index_edges()
    assert tri.max() == MC.BIG_NV - 1 and tri.min() >= 0
    lab, _ = _agree(tri, "edge keys up to 2^31 - 2")
    assert lab.tolist() == MC.BIG_INDEX_EDGE_LABELS


def test_area_cases():
    v, tri = MC.isolated_with_areas(65)
    a = MR.triangle_areas(v, tri)
    assert a[0] == 0.0 and a[1] == 0.0 and a[2] == 0.0 and np.isfinite(a).all() and (a[5:] > 0).all()
    v, tri = MC.area_fan()
    assert len(tri) == 4096
    lab, sizes, terms = MR.cluster_connected_triangles(v, tri)
    assert sizes.tolist() == [4096] and len(terms) == 1
    assert terms[0].min() < 2e-12 and terms[0].max() > 5e2  # spread over 1e-12 .. 1e3
    s, bound = MR.area_bound(terms[0])
    assert 0 < bound < 1e-9 * s


def test_duplicate_rules():
    tri = MC.duplicate_basics()
    mask = MR.duplicated_mask(tri)
    assert np.nonzero(mask)[0].tolist() == MC.DUPLICATE_BASICS_REMOVED
    out = MR.remove_duplicated_triangles(tri)
    assert out[0].tolist() == [2, 0, 1]  # the survivor keeps its own rotation
    assert MR.canonical_key(3, 7, 3) == (3, 7, 3) and MR.canonical_key(3, 3, 7) == MR.canonical_key(7, 3, 3) == (3, 3, 7)
    assert MR.canonical_key(0, 2, 1) != MR.canonical_key(0, 1, 2)
    for n in (257, 1025, 4000):
        t = MC.duplicate_runs(n)
        m = MR.duplicated_mask(t)
        keys = [MR.canonical_key(*r) for r in t.tolist()]
        assert max(keys.count(k) for k in set(keys[:50])) >= 3
        assert m.sum() == n - len(set(keys))
    t, survivors = MC.big_index_duplicates()
    assert t.max() == MC.BIG_NV - 1 and t.min() >= 0
    assert len(MR.remove_duplicated_triangles(t)) == survivors


def test_cleanup_reference_on_the_sizes():
    for n in MC.SIZES:
        nv, tri = MC.cleanup_soup(n)
        assert tri.max() == nv - 1
        v = MC.random_vertices(nv, n)
        v2, t2, c2, n2, kept = MR.remove_unreferenced_vertices(v, tri, colors=v + 1.0)
        assert kept[-1] == nv - 1 and len(kept) < nv
        assert_bitwise(v2[t2], v[tri], "the triangles still name the same points")
        assert_bitwise(c2, v2 + 1.0, "colours follow")
        again = MR.remove_unreferenced_vertices(v2, t2)
        assert_bitwise(again[0], v2, "a second call is the identity")
        assert_bitwise(again[1], t2, "a second call is the identity")
        for name, m in MC.masks(n).items():
            assert len(MR.remove_triangles_by_mask(tri, m)) == int((~m).sum()), name
        assert_bitwise(MR.remove_triangles_by_index(tri, [-1, 0, 0, n, n - 1]),
                       MR.remove_triangles_by_mask(tri, np.isin(np.arange(n), [0, n - 1])), "by index")


def test_two_sphere_volume_is_small():
    keys, tsdf, weight, color = MC.two_spheres()
    assert keys.shape == (8, 3) and tsdf.shape == (8, 4096)
    assert (tsdf < 0).any() and (tsdf > 0).any()


# ------------------------------------------------------------------------------------------------ the interface
def test_header_declares_and_table_binds_the_entries(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.native_library()
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bot_status\s+" + name + r"\s*\(", src), name
        assert len(pkg._lib.SIGNATURES[name]) == nargs, name
        assert name not in lib._ot_missing
    assert lib.ot_abi_version() == 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_c_abi_argument_errors_need_no_device(pkg):
    lib = pkg.native_library()
    bad = pkg._lib.OT_ERR_INVALID_ARGUMENT
    tri = np.zeros((4, 3), np.int32)
    out = np.zeros((4, 3), np.int32)
    lab, cnt, mask = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    area, v = np.zeros(4), np.zeros((3, 3))
    k = C.c_int64(7)
    big = 2 ** 31 // 3 + 1
    calls = [
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            None, 4, _p(v), 3, _p(lab), _p(cnt), _p(area), C.byref(k), None)),
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), 4, _p(v), 3, None, _p(cnt), _p(area), C.byref(k), None)),
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), 4, _p(v), 3, _p(lab), _p(cnt), None, C.byref(k), None)),  # vertices without areas
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), 4, None, 3, _p(lab), _p(cnt), _p(area), C.byref(k), None)),  # areas without vertices
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), -1, _p(v), 3, _p(lab), _p(cnt), _p(area), C.byref(k), None)),
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), big, _p(v), 3, _p(lab), _p(cnt), _p(area), C.byref(k), None)),
        ("ClusterConnectedTriangles", lambda: lib.ot_mesh_cluster_connected_triangles(
            _p(tri), 4, _p(v), 2 ** 31, _p(lab), _p(cnt), _p(area), C.byref(k), None)),
        ("RemoveDegenerateTriangles", lambda: lib.ot_mesh_flag_degenerate_triangles(_p(tri), 4, 3, None, None)),
        ("RemoveDegenerateTriangles", lambda: lib.ot_mesh_flag_degenerate_triangles(_p(tri), 4, -1, _p(mask), None)),
        ("RemoveDuplicatedTriangles", lambda: lib.ot_mesh_flag_duplicated_triangles(None, 4, 3, _p(mask), None)),
        ("RemoveDuplicatedTriangles", lambda: lib.ot_mesh_flag_duplicated_triangles(_p(tri), big, 3, _p(mask), None)),
        ("RemoveTrianglesByMask", lambda: lib.ot_mesh_remove_triangles_by_mask(
            _p(tri), 4, None, _p(out), C.byref(k), None)),
        ("RemoveTrianglesByMask", lambda: lib.ot_mesh_remove_triangles_by_mask(
            _p(tri), 4, _p(mask), _p(tri), C.byref(k), None)),  # output aliases the input
        ("RemoveTrianglesByMask", lambda: lib.ot_mesh_remove_triangles_by_mask(
            _p(tri), 4, _p(mask), _p(out), None, None)),
        ("RemoveTrianglesByMask", lambda: lib.ot_mesh_remove_triangles_by_mask(
            _p(tri), -4, _p(mask), _p(out), C.byref(k), None)),
        ("RemoveUnreferencedVertices", lambda: lib.ot_mesh_remove_unreferenced_vertices(
            3, None, 4, _p(lab), C.byref(k), None)),
        ("RemoveUnreferencedVertices", lambda: lib.ot_mesh_remove_unreferenced_vertices(
            3, _p(tri), 4, None, C.byref(k), None)),
        ("RemoveUnreferencedVertices", lambda: lib.ot_mesh_remove_unreferenced_vertices(
            -3, _p(tri), 4, _p(lab), C.byref(k), None)),
    ]
    for who, call in calls:
        assert call() == bad, who
        assert lib.ot_last_error().decode().startswith("[" + who + "]"), lib.ot_last_error()


def test_empty_inputs_need_no_device(pkg):
    lib = pkg.native_library()
    k = C.c_int64(7)
    assert lib.ot_mesh_cluster_connected_triangles(None, 0, None, 0, None, None, None, C.byref(k), None) == 0
    assert k.value == 0
    assert lib.ot_mesh_flag_degenerate_triangles(None, 0, 0, None, None) == 0
    assert lib.ot_mesh_flag_duplicated_triangles(None, 0, 5, None, None) == 0
    k = C.c_int64(7)
    assert lib.ot_mesh_remove_triangles_by_mask(None, 0, None, None, C.byref(k), None) == 0
    assert k.value == 0
    k = C.c_int64(7)
    assert lib.ot_mesh_remove_unreferenced_vertices(0, None, 0, None, C.byref(k), None) == 0
    assert k.value == 0
    G, U = pkg.geometry, pkg.utility
    mesh = G.TriangleMesh()
    labels, sizes, areas = mesh.cluster_connected_triangles()
    assert isinstance(labels, U.IntVector) and isinstance(areas, U.DoubleVector) and isinstance(sizes, list)
    assert len(labels) == len(sizes) == len(areas) == 0
    for call in (mesh.remove_degenerate_triangles, mesh.remove_duplicated_triangles, mesh.remove_unreferenced_vertices,
                 lambda: mesh.remove_triangles_by_mask([]), lambda: mesh.remove_triangles_by_index([0, 5])):
        assert call() is mesh
    assert len(mesh.triangles) == 0 and len(mesh.vertices) == 0


def test_mask_length_error_needs_no_device(pkg):
    G = pkg.geometry
    mesh = G.TriangleMesh(np.zeros((3, 3)), np.array([[0, 1, 2], [0, 2, 1]], np.int32))
    for mask in ([True], [True, False, True], []):
        with pytest.raises(RuntimeError, match=r"\[RemoveTrianglesByMask\] triangle_mask needs to have same size as "
                                               r"triangles_\."):
            mesh.remove_triangles_by_mask(mask)
    with pytest.raises(RuntimeError, match=r"\[RemoveTrianglesByMask\]"):
        MR.remove_triangles_by_mask(np.zeros((2, 3), np.int32), [True])
    assert len(mesh.triangles) == 2
