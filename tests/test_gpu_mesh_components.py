"""GPU parity of TriangleMesh.cluster_connected_triangles, remove_triangles_by_mask / _by_index,
remove_unreferenced_vertices, remove_degenerate_triangles and remove_duplicated_triangles (csrc/mesh_components.hip)
against the sequential reference of tests/mesh_components_ref.py: labels, counts, surviving triangles, vertices,
colours, normals and kept-index maps bit for bit; the area of a one-triangle cluster bit for bit, the area sum of a
larger cluster within n * 2^-52 * fsum (derived in DESIGN.md §4, not measured).  The designed meshes are those of
tests/mesh_component_cases.py, whose properties test_mesh_components_api.py asserts on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_component_cases as MC
import mesh_components_ref as MR
from conftest import assert_bitwise

pytestmark = pytest.mark.gpu


def _mesh(pkg, tri, v=None, colors=None, normals=None):
    if v is None:
        v = MC.random_vertices(MC.vertex_count(tri), 5)
    m = pkg.geometry.TriangleMesh(v, tri)
    if colors is not None:
        m.vertex_colors = pkg.utility.Vector3dVector(colors)
    if normals is not None:
        m.vertex_normals = pkg.utility.Vector3dVector(normals)
    return m


def _tri(mesh):
    return np.asarray(mesh.triangles, np.int32).reshape(-1, 3)


def _cluster(pkg, tri, v=None):
    mesh = _mesh(pkg, tri, v)
    labels, sizes, areas = mesh.cluster_connected_triangles()
    assert isinstance(labels, pkg.utility.IntVector) and len(labels) == len(tri)
    assert isinstance(sizes, list) and all(type(n) is int for n in sizes[:16])
    assert all(type(x) is int for x in labels[:16])
    assert isinstance(areas, pkg.utility.DoubleVector) and len(areas) == len(sizes)
    return mesh, np.asarray(labels, np.int32), sizes, np.asarray(areas)


def _check_areas(got, terms, what):
    assert len(got) == len(terms)
    single = np.array([len(t) == 1 for t in terms], bool)
    if single.any():
        want = np.array([t[0] for t, s in zip(terms, single) if s])
        assert_bitwise(got[single], want, what + ": areas of one-triangle clusters")
    for k in np.nonzero(~single)[0]:
        s, bound = MR.area_bound(terms[k])
        err = abs(float(got[k]) - s)
        assert err <= bound, f"{what}: cluster {k} of {len(terms[k])}: |{got[k]!r} - {s!r}| = {err} > {bound}"


def _check(pkg, tri, what, v=None):
    assert len(tri) <= 5000
    if v is None:
        v = MC.random_vertices(MC.vertex_count(tri), 5)
    ref_l, ref_n, terms = MR.cluster_connected_triangles(v, tri)
    mesh, labels, sizes, areas = _cluster(pkg, tri, v)
    assert_bitwise(labels, ref_l, what + ": labels")
    assert_bitwise(np.asarray(sizes, np.int32), ref_n, what + ": cluster sizes")
    _check_areas(areas, terms, what)
    assert_bitwise(_tri(mesh), tri, what + ": the clustering leaves the triangles alone")
    return ref_l, sizes


# ------------------------------------------------------------------------------------------------- connectivity
def test_random_soups_and_permutations(pkg, gpu):
    rng = np.random.default_rng(41)
    for i, tri in enumerate(MC.random_soups(2, 30)):
        _check(pkg, tri, f"soup {i}")
        _check(pkg, tri[rng.permutation(len(tri))], f"soup {i} permuted")


def test_bow_ties_and_edge_direction(pkg, gpu):
    lab, _ = _check(pkg, MC.bow_tie(), "bow-tie")
    assert lab.tolist() == [0, 1]
    lab, _ = _check(pkg, MC.bow_tie_fan(100), "fan of 100 bow-ties")
    assert lab.tolist() == list(range(100))
    lab, _ = _check(pkg, MC.opposite_edges(), "opposite and equal edge directions")
    assert lab.tolist() == [0, 0, 1, 1, 2]


def test_nonmanifold_edges(pkg, gpu):
    for k in (5, 300):
        _, sizes = _check(pkg, MC.shared_edge(k), f"one edge shared by {k}")
        assert sizes == [k]
    tri = MC.nonmanifold_runs()
    _, sizes = _check(pkg, tri, "runs of 300 equal keys across positions 256 and 1024")
    assert sizes == [1] * MC.NM_FILL + [MC.NM_RUN] * 2
    _check(pkg, tri[np.random.default_rng(43).permutation(len(tri))], "the same, permuted")


def test_degenerate_triangles_link(pkg, gpu):
    lab, _ = _check(pkg, MC.degenerate_links(), "(a, a, b), (a, a, c) and (a, a, a)")
    assert lab.tolist() == MC.DEGENERATE_LINK_LABELS


# ------------------------------------------------------------------------------------------- no iteration cap
def test_strips(pkg, gpu):
    s = MC.strip(4096)
    rng = np.random.default_rng(47)
    for name, t in (("index order", s), ("reversed", np.ascontiguousarray(s[::-1])),
                    ("permuted", s[rng.permutation(len(s))])):
        lab, sizes = _check(pkg, t, f"strip of 4096, {name}")
        assert sizes == [4096] and (lab == 0).all()
    lab, sizes = _check(pkg, MC.two_strips(), "two interleaved strips")
    assert sizes == [2048, 2048] and (lab[0::2] == 0).all() and (lab[1::2] == 1).all()


def test_numbering_by_smallest_triangle_index(pkg, gpu):
    lab, _ = _check(pkg, MC.numbering(), "numbering")
    assert lab.tolist() == [0, 0, 1, 1]


# -------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", MC.SIZES)
def test_sizes_isolated_triangles(pkg, gpu, n):
    v, tri = MC.isolated_with_areas(n)
    lab, sizes = _check(pkg, tri, f"{n} isolated triangles", v)  # every area is a one-triangle cluster's: bit for bit
    assert lab.tolist() == list(range(n)) and sizes == [1] * n


def test_no_triangles(pkg, gpu):
    mesh = _mesh(pkg, np.zeros((0, 3), np.int32), MC.random_vertices(5, 1))
    labels, sizes, areas = mesh.cluster_connected_triangles()
    assert len(labels) == len(sizes) == len(areas) == 0
    assert mesh.remove_degenerate_triangles() is mesh and mesh.remove_duplicated_triangles() is mesh
    assert mesh.remove_triangles_by_mask([]) is mesh
    assert mesh.remove_unreferenced_vertices() is mesh
    assert len(mesh.vertices) == 0 and len(mesh.triangles) == 0  # nothing references a vertex


@pytest.mark.parametrize("n", MC.SIZES)
def test_sizes_cleanup_calls(pkg, gpu, n):
    nv, tri = MC.cleanup_soup(n)
    v = MC.random_vertices(nv, n)
    col, nrm = v * 0.5 + 0.25, v[:, ::-1] * 3.0
    m = _mesh(pkg, tri, v)
    assert m.remove_degenerate_triangles() is m
    assert_bitwise(_tri(m), MR.remove_degenerate_triangles(tri), f"degenerate, T = {n}")
    m = _mesh(pkg, tri, v)
    assert m.remove_duplicated_triangles() is m
    assert_bitwise(_tri(m), MR.remove_duplicated_triangles(tri), f"duplicated, T = {n}")
    for name, mask in MC.masks(n).items():
        m = _mesh(pkg, tri, v, col, nrm)
        assert m.remove_triangles_by_mask(mask.tolist()) is m
        assert_bitwise(_tri(m), MR.remove_triangles_by_mask(tri, mask), f"mask {name}, T = {n}")
        assert_bitwise(np.asarray(m.vertices), v, "a triangle call leaves the vertices alone")
        assert_bitwise(np.asarray(m.vertex_colors), col, "and the colours")
        assert_bitwise(np.asarray(m.vertex_normals), nrm, "and the normals")
    idx = [-1, 0, 0, n, n - 1, n // 2, 10 ** 9]
    m = _mesh(pkg, tri, v)
    assert m.remove_triangles_by_index(idx) is m
    assert_bitwise(_tri(m), MR.remove_triangles_by_index(tri, idx), f"by index, T = {n}")
    m = _mesh(pkg, tri, v, col, nrm)
    assert m.remove_unreferenced_vertices() is m
    v2, t2, c2, n2, kept = MR.remove_unreferenced_vertices(v, tri, col, nrm)
    assert_bitwise(_tri(m), t2, f"unreferenced: triangles, T = {n}")
    assert_bitwise(np.asarray(m.vertices), v2, "unreferenced: vertices")
    assert_bitwise(np.asarray(m.vertex_colors), c2, "unreferenced: colours")
    assert_bitwise(np.asarray(m.vertex_normals), n2, "unreferenced: normals")


# -------------------------------------------------------------------------------------------------------- areas
def test_area_of_a_large_cluster_and_determinism(pkg, gpu):
    v, tri = MC.area_fan()
    ref_l, ref_n, terms = MR.cluster_connected_triangles(v, tri)
    assert ref_n.tolist() == [4096]
    _, labels, sizes, a = _cluster(pkg, tri, v)
    assert_bitwise(labels, ref_l, "area fan: labels")
    assert sizes == [4096]
    s, bound = MR.area_bound(terms[0])
    print(f"area fan: got {a[0]!r}, fsum {s!r}, |difference| {abs(a[0] - s)!r}, bound {bound!r}")
    assert abs(float(a[0]) - s) <= bound == 4096 * 2.0 ** -52 * math.fsum(terms[0].tolist())
    _, _, _, b = _cluster(pkg, tri, v)
    assert_bitwise(a, b, "two calls give identical bits")
    tri2 = MC.nonmanifold_runs()
    v2 = MC.random_vertices(MC.vertex_count(tri2), 9)
    a2, b2 = _cluster(pkg, tri2, v2)[3], _cluster(pkg, tri2, v2)[3]
    assert_bitwise(a2, b2, "two calls give identical bits (36 clusters)")


# --------------------------------------------------------------------------------------------------- duplicates
def test_duplicate_rules(pkg, gpu):
    tri = MC.duplicate_basics()
    m = _mesh(pkg, tri)
    m.remove_duplicated_triangles()
    want = MR.remove_duplicated_triangles(tri)
    assert_bitwise(_tri(m), want, "rotations, a flip, the (a, b, a) quirk")
    assert_bitwise(want, np.delete(tri, MC.DUPLICATE_BASICS_REMOVED, axis=0), "the survivors keep rotation and order")
    for n in (257, 1025, 4000):
        t = MC.duplicate_runs(n)
        m = _mesh(pkg, t)
        m.remove_duplicated_triangles()
        assert_bitwise(_tri(m), MR.remove_duplicated_triangles(t), f"runs of duplicates across blocks, T = {n}")


def _dev(pkg, a):
    return pkg._device.to_device(np.ascontiguousarray(a))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def test_big_indices_through_the_c_abi(pkg, gpu):
    """n_vertices = 2^31 - 1 and no vertex array: the 96-bit duplicate key and the 62-bit edge key in full"""
    import torch

    lib, D = pkg.native_library(), pkg._device
    s = D.stream_ptr()
    tri, survivors = MC.big_index_duplicates()
    dt = _dev(pkg, tri)
    mask = torch.zeros(len(tri), dtype=torch.uint8, device=dt.device)
    assert lib.ot_mesh_flag_duplicated_triangles(_ptr(dt), len(tri), MC.BIG_NV, _ptr(mask), s) == 0, lib.ot_last_error()
    want = MR.duplicated_mask(tri)
    assert_bitwise(mask.cpu().numpy().astype(bool), want, "duplicate mask, indices up to 2^31 - 2")
    assert int((~want).sum()) == survivors
    out = torch.zeros((len(tri), 3), dtype=torch.int32, device=dt.device)
    k = C.c_int64(0)
    assert lib.ot_mesh_remove_triangles_by_mask(_ptr(dt), len(tri), _ptr(mask), _ptr(out), C.byref(k), s) == 0
    assert_bitwise(out[:k.value].cpu().numpy(), MR.remove_duplicated_triangles(tri), "survivors, big indices")
    dmask = torch.zeros(len(tri), dtype=torch.uint8, device=dt.device)
    assert lib.ot_mesh_flag_degenerate_triangles(_ptr(dt), len(tri), MC.BIG_NV, _ptr(dmask), s) == 0
    assert_bitwise(dmask.cpu().numpy().astype(bool), MR.degenerate_mask(tri), "degenerate mask, big indices")

    tri = MC.big_index_edges()
    dt = _dev(pkg, tri)
    labels = torch.zeros(len(tri), dtype=torch.int32, device=dt.device)
    counts = torch.zeros(len(tri), dtype=torch.int32, device=dt.device)
    k = C.c_int64(0)
    assert lib.ot_mesh_cluster_connected_triangles(_ptr(dt), len(tri), None, MC.BIG_NV, _ptr(labels), _ptr(counts),
                                                   None, C.byref(k), s) == 0, lib.ot_last_error()
    ref_l, ref_n = MR.cluster_closed(tri)
    assert_bitwise(labels.cpu().numpy(), ref_l, "edge keys up to 2^31 - 2: labels")
    assert ref_l.tolist() == MC.BIG_INDEX_EDGE_LABELS
    assert counts[:k.value].cpu().numpy().tolist() == ref_n


# ---------------------------------------------------------------------------------------------- compaction calls
def test_unreferenced_vertices(pkg, gpu):
    import torch

    v = MC.random_vertices(300, 3)
    col, nrm = v + 2.0, -v
    none = _mesh(pkg, np.zeros((0, 3), np.int32), v, col, nrm)
    none.remove_unreferenced_vertices()
    assert len(none.vertices) == len(none.vertex_colors) == len(none.vertex_normals) == 0
    every = np.ascontiguousarray(np.arange(300, dtype=np.int32)[::-1].reshape(100, 3))
    last = np.array([[299, 299, 299]], np.int32)
    some = np.array([[298, 7, 130], [7, 7, 299], [130, 256, 255]], np.int32)
    for name, tri in (("everything referenced", every), ("only the last vertex", last), ("a few", some)):
        m = _mesh(pkg, tri, v, col, nrm)
        assert m.remove_unreferenced_vertices() is m
        v2, t2, c2, n2, kept = MR.remove_unreferenced_vertices(v, tri, col, nrm)
        assert_bitwise(np.asarray(m.vertices), v2, name + ": vertices")
        assert_bitwise(_tri(m), t2, name + ": triangles")
        assert_bitwise(np.asarray(m.vertex_colors), c2, name + ": colours")
        assert_bitwise(np.asarray(m.vertex_normals), n2, name + ": normals")
        m.remove_unreferenced_vertices()
        assert_bitwise(np.asarray(m.vertices), v2, name + ": a second call is the identity")
        assert_bitwise(_tri(m), t2, name + ": a second call is the identity")
        assert_bitwise(np.asarray(m.vertex_normals), n2, name + ": a second call is the identity")
        # the kept-index map itself, through the C ABI
        lib, s = pkg.native_library(), pkg._device.stream_ptr()
        dt = _dev(pkg, tri)
        kept_d = torch.full((300,), -7, dtype=torch.int32, device=dt.device)
        k = C.c_int64(0)
        assert lib.ot_mesh_remove_unreferenced_vertices(300, _ptr(dt), len(tri), _ptr(kept_d), C.byref(k), s) == 0
        assert_bitwise(kept_d[:k.value].cpu().numpy(), kept, name + ": kept old index")
        assert (kept_d[k.value:] == -7).all()
        assert_bitwise(dt.cpu().numpy(), t2, name + ": triangles rewritten in place")


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", ["n_vertices", -1])
def test_out_of_range_index_is_refused(pkg, gpu, bad):
    import torch

    lib, s = pkg.native_library(), pkg._device.stream_ptr()
    good = MC.nonmanifold_runs()
    nv = MC.vertex_count(good)
    tri = good.copy()
    tri[len(tri) // 2, 1] = nv if bad == "n_vertices" else -1
    dt = _dev(pkg, tri)
    labels = torch.zeros(len(tri), dtype=torch.int32, device=dt.device)
    counts = torch.zeros(len(tri), dtype=torch.int32, device=dt.device)
    mask = torch.zeros(len(tri), dtype=torch.uint8, device=dt.device)
    kept = torch.zeros(nv, dtype=torch.int32, device=dt.device)
    k = C.c_int64(0)
    refused = pkg._lib.OT_ERR_INVALID_ARGUMENT
    calls = (
        ("ClusterConnectedTriangles", lambda t: lib.ot_mesh_cluster_connected_triangles(
            _ptr(t), len(tri), None, nv, _ptr(labels), _ptr(counts), None, C.byref(k), s)),
        ("RemoveDegenerateTriangles", lambda t: lib.ot_mesh_flag_degenerate_triangles(_ptr(t), len(tri), nv, _ptr(mask), s)),
        ("RemoveDuplicatedTriangles", lambda t: lib.ot_mesh_flag_duplicated_triangles(_ptr(t), len(tri), nv, _ptr(mask), s)),
        ("RemoveUnreferencedVertices", lambda t: lib.ot_mesh_remove_unreferenced_vertices(
            nv, _ptr(t), len(tri), _ptr(kept), C.byref(k), s)),
    )
    for who, call in calls:
        assert call(dt) == refused, who
        assert lib.ot_last_error().decode() == f"[{who}] triangle index out of range [0, n_vertices)"
        assert_bitwise(dt.cpu().numpy(), tri, who + ": a refused call changes nothing")
    for who, call in calls:  # the next valid call still works
        assert call(_dev(pkg, good)) == 0, who
    assert_bitwise(labels.cpu().numpy(), MR.cluster_closed(good)[0], "labels after the refusals")
    m = _mesh(pkg, tri, MC.random_vertices(nv, 1))
    for method in (m.cluster_connected_triangles, m.remove_degenerate_triangles, m.remove_duplicated_triangles,
                   m.remove_unreferenced_vertices):
        with pytest.raises(RuntimeError, match=r"triangle index out of range \[0, n_vertices\)"):
            method()
    assert_bitwise(_tri(m), tri, "a refused facade call leaves the mesh alone")
    _check(pkg, good, "the facade after the refusals")


# ----------------------------------------------------------------------------------------------- recipe end to end
def test_recipe_on_an_extracted_mesh(pkg, gpu):
    """cluster -> mask of the small clusters -> remove_triangles_by_mask -> remove_unreferenced_vertices on the
    marching-cubes mesh of a volume holding two separate surfaces"""
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = MC.two_spheres()
    vol = integ.ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8,
                                   color_precision=64, max_units=64)
    vol.import_units(keys, tsdf, weight, color)
    first = vol.extract_triangle_mesh()
    first.compute_vertex_normals()
    V, VC, VN, T = (np.array(a) for a in (first.vertices, first.vertex_colors, first.vertex_normals, first.triangles))
    T = T.astype(np.int32)
    assert 1000 < len(T) <= 20000

    mesh = vol.extract_triangle_mesh()  # fresh: its vertex normals are the deferred marching-cubes walk
    mesh.compute_vertex_normals()
    labels, sizes, areas = mesh.cluster_connected_triangles()
    ref_l, ref_n, terms = MR.cluster_connected_triangles(V, T)
    print(f"two spheres: {len(V)} vertices, {len(T)} triangles, cluster sizes {sizes}")
    assert_bitwise(np.asarray(labels, np.int32), ref_l, "extracted mesh: labels")
    assert_bitwise(np.asarray(sizes, np.int32), ref_n, "extracted mesh: cluster sizes")
    _check_areas(np.asarray(areas), terms, "extracted mesh")
    assert len(sizes) >= 2
    k = max(sizes)
    mask = np.asarray(sizes)[np.asarray(labels)] < k
    assert 0 < mask.sum() < len(T)
    assert mesh.remove_triangles_by_mask(mask) is mesh
    T1 = MR.remove_triangles_by_mask(T, mask)
    assert_bitwise(_tri(mesh), T1, "recipe: surviving triangles")
    assert mesh.remove_unreferenced_vertices() is mesh
    V2, T2, C2, N2, kept = MR.remove_unreferenced_vertices(V, T1, VC, VN)
    assert len(V2) < len(V)
    assert_bitwise(_tri(mesh), T2, "recipe: rewritten triangles")
    assert_bitwise(np.asarray(mesh.vertices), V2, "recipe: vertices")
    assert_bitwise(np.asarray(mesh.vertex_colors), C2, "recipe: colours")
    assert_bitwise(np.asarray(mesh.vertex_normals), N2, "recipe: normals carried through")
    assert mesh.cluster_connected_triangles()[1] == [k]
    assert mesh._mc is None
    mesh.compute_vertex_normals()  # the generic path: the arrays are no longer the extraction's
    generic = pkg.geometry.TriangleMesh(V2, T2).compute_vertex_normals()
    assert_bitwise(np.asarray(mesh.vertex_normals), np.asarray(generic.vertex_normals), "recipe: normals recomputed")
    pts = np.asarray(mesh.sample_points_uniformly(1000, seed=3).points)
    assert pts.shape == (1000, 3) and np.isfinite(pts).all()
