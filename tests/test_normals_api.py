"""PointCloud.estimate_normals and friends without a device: the numpy reference (tests/normals_ref.py) against
numpy.linalg.eigh on every designed cloud of test_gpu_normals.py, the properties those clouds were designed for, the
search-parameter classes, the refusals (raised before any device work), and the C ABI declaration and binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normals_clouds as NC
import normals_ref as NR
from conftest import ROOT, assert_bitwise

ALL = sorted(NC.cases())


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", ALL)
def test_reference_agrees_with_eigh(name):
    """Up to sign, on every trigonometric-path point whose two smallest eigenvalues are separated by >= 1e-3 of the
    largest.  An eigenvector moves by about (error of the matrix) / gap; the solver and eigh each work to a few dozen
    eps on a matrix scaled to 1, so 2 x 64 x 2^-53 / 1e-3 = 1.4e-11 rad bounds their disagreement; 1e-10 is asserted."""
    pts, k, radius, prior = NC.cases()[name]
    ref = NC.reference(name)
    assert len(ref["nbrs"]) == len(pts) and ref["cov"].shape == (len(pts), 3, 3)
    mask = (ref["path"] == NR.PATH_TRIG) & (ref["gap"] >= 1e-3)
    worst = 0.0
    for i in np.nonzero(mask)[0]:
        w, Q = np.linalg.eigh(ref["cov"][i])
        worst = max(worst, float(NR.angle(ref["normals"][i], Q[:, 0])))
    print(f"{name}: {int(mask.sum())} of {len(pts)} points compared, largest angle to eigh {worst:.3g} rad")
    assert worst <= 1e-10
    n2 = (ref["normals"] ** 2).sum(axis=1)
    nonzero = n2 > 0
    assert np.abs(n2[nonzero] - 1.0).max(initial=0.0) < 1e-12  # unit normals (zero only from a zero prior)
    if prior is None:
        assert nonzero.all()


@pytest.mark.parametrize("name", [n for n in ALL if n not in NC.EXEMPT_FROM_GAP_RULE])
def test_gap_rule_leaves_out_at_most_5_percent(name):
    ref = NC.reference(name)
    trig = ref["path"] == NR.PATH_TRIG
    left_out = int((trig & (ref["gap"] < 1e-3)).sum())
    assert left_out <= 0.05 * len(ref["path"]), f"{left_out} of {len(ref['path'])} points below the gap"
    mask, limit, worst = NC.tolerance(ref)
    print(f"{name}: {left_out} left out, float64 vs long double {worst:.3g} rad, limit {limit:.3g} rad")
    assert limit < 1e-9  # the reference itself is well conditioned where it is compared


def test_neighbour_order_and_hybrid_filter():
    pts, k, radius, _ = NC.cases()["box_hybrid"]
    ref = NC.reference("box_hybrid")
    knn = NC.reference("box_k30")
    r2 = np.float64(radius) * np.float64(radius)
    for i in (0, 1, 500, 777, 1499):
        full = knn["nbrs"][i]
        assert full[0] == i and len(full) == 30
        d2 = ((pts[full] - pts[i]) ** 2).sum(axis=1)
        assert (np.diff(d2) >= -1e-18).all()
        assert ref["nbrs"][i].tolist() == [j for j in full if _d2(pts[i], pts[j]) < r2]
    counts = np.array([len(nb) for nb in ref["nbrs"]])
    assert (counts < 3).any() and (counts >= 3).sum() > 1000 and counts.max() < 30  # the radius binds everywhere
    k5 = np.array([len(nb) for nb in NC.reference("box_hybrid_k5")["nbrs"]])
    assert (k5 == 5).sum() > 500 and (k5 < 5).sum() > 100  # max_nn binds for some points, the radius for others
    assert (k5 == np.minimum(counts, 5)).all()
    few = counts < 3
    assert (ref["path"][few] == NR.PATH_FEW).all() and (ref["path"][~few] != NR.PATH_FEW).all()
    assert_bitwise(ref["cov"][few], np.broadcast_to(np.eye(3), (int(few.sum()), 3, 3)), "identity below 3 neighbours")
    assert_bitwise(ref["normals"][few], np.broadcast_to([0.0, 0.0, 1.0], (int(few.sum()), 3)), "+z below 3")


def _d2(a, b):
    d = b - a
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def test_permutation_changes_indices_only():
    a, b = NC.reference("box_k30"), NC.reference("box_permuted")
    perm = np.random.default_rng(8).permutation(1500)
    # no two distances tie in the noisy cloud, so the neighbour sets map through the permutation
    for i in (0, 3, 1499):
        assert sorted(perm[b["nbrs"][i]].tolist()) == sorted(a["nbrs"][perm[i]].tolist())


def test_lattice():
    ref = NC.reference("lattice_k16")
    # a symmetric neighbourhood has no xy term (the diagonal path), the index rule skews the others (trigonometric)
    assert set(ref["path"].tolist()) == {NR.PATH_DIAGONAL, NR.PATH_TRIG}
    # every sum is exact and the z row of C is zero: x and y of the normal are exact zeros; |z| is 1 on the diagonal
    # path and the product of two normalised in-plane vectors on the other (1 or 1 - 2^-52)
    assert (ref["normals"][:, :2] == 0).all()
    assert (np.abs(np.abs(ref["normals"][:, 2]) - 1.0) <= 2.0 ** -52).all()
    assert (np.abs(ref["normals"][ref["path"] == NR.PATH_DIAGONAL, 2]) == 1.0).all()
    assert (ref["cov"][:, 2, :] == 0).all() and (ref["cov"][:, :, 2] == 0).all()
    # ties everywhere: the 16 neighbours of a corner are decided by the index rule
    pts = NC.lattice()
    d2 = ((pts - pts[0]) ** 2).sum(axis=1)
    kth = np.sort(d2)[15]
    assert (d2 == kth).sum() > 1 and (d2 <= kth).sum() > 16
    at = NC.reference("lattice_hybrid_at_spacing")  # strict <: a neighbour at exactly the radius is left out
    assert all(nb.tolist() == [i] for i, nb in enumerate(at["nbrs"]))
    assert (at["path"] == NR.PATH_FEW).all()
    above = NC.reference("lattice_hybrid_above_spacing")
    counts = np.array([len(nb) for nb in above["nbrs"]])
    assert counts.max() == 5 and counts.min() == 3 and (counts == 5).sum() == 100


def test_coincident_groups():
    pts, gid = NC.coincident()
    ref = NC.reference("coincident_k8")
    for i in range(len(pts)):
        assert ref["nbrs"][i].tolist() == np.nonzero(gid == gid[i])[0][:8].tolist()  # lowest index first
    dyadic = gid < 3
    assert (ref["path"][dyadic] == NR.PATH_ZERO).all()
    assert (ref["cov"][dyadic] == 0).all()
    assert_bitwise(ref["normals"][dyadic], np.broadcast_to([0.0, 0.0, 1.0], (int(dyadic.sum()), 3)), "zero matrix: +z")
    pr = NC.cases()["coincident_priors"][3]
    withp = NC.reference("coincident_priors")
    assert_bitwise(withp["normals"][dyadic], pr[dyadic], "zero matrix: the prior normal, a zero prior included")
    assert (withp["normals"][:3] == 0).all()


def test_prior_normals_orient_the_result():
    pts, k, radius, pr = NC.cases()["box_priors"]
    ref = NC.reference("box_priors")
    dots = (ref["normals"] * pr).sum(axis=1)
    assert (dots >= 0).all()
    zero = (pr == 0).all(axis=1)
    assert zero.sum() == 3 and (np.abs((ref["normals"][zero] ** 2).sum(axis=1) - 1) < 1e-12).all()
    plain = NR.estimate(pts, k, None, None)["normals"]
    flipped = (plain * pr).sum(axis=1) < 0
    assert flipped.sum() > 50 and (~flipped).sum() > 50
    assert_bitwise(ref["normals"][flipped], -plain[flipped], "negated where the prior points the other way")
    assert_bitwise(ref["normals"][~flipped], plain[~flipped], "kept elsewhere")


def test_line_far_point_and_small_clouds():
    ref = NC.reference("line_k10")
    w = np.linalg.eigvalsh(ref["cov"])
    assert (w[:, 1] < 1e-9 * w[:, 2]).all()  # rank one: the two smallest eigenvalues coincide
    far = NC.reference("far_point_k30")
    assert far["nbrs"][500][0] == 500 and len(far["nbrs"][500]) == 30
    for n in (1, 2):
        assert (NC.reference(f"n{n}_k30")["path"] == NR.PATH_FEW).all()
    assert (NC.reference("n3_k30")["path"] != NR.PATH_FEW).all()
    assert all(len(nb) == 29 for nb in NC.reference("n29_k30")["nbrs"])
    assert all(len(nb) == 30 for nb in NC.reference("n31_k30")["nbrs"])
    assert (NC.reference("n257_k2")["path"] == NR.PATH_FEW).all()
    assert (NC.reference("n257_k3")["path"] != NR.PATH_FEW).all()
    for axis in range(3):
        counts = np.array([len(nb) for nb in NC.reference(f"straddle_hybrid_axis{axis}")["nbrs"]])
        assert (counts == 2).sum() >= 400 and (counts == 1).sum() >= 2  # both outcomes of the strict <


def test_orientation_reference():
    N = np.array([[0.0, 0.0, 0.0], [0.0, 0.6, -0.8], [1.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    P = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    d = NR.orient_to_direction(N, (0.0, 0.0, 1.0))
    assert d.tolist() == [[0.0, 0.0, 1.0], [-0.0, -0.6, 0.8], [1.0, 0.0, 0.0], [0.0, 0.0, 2.0]]
    c = NR.orient_to_camera(N, P, (1.0, 1.0, 1.0))
    assert c[0].tolist() == [0.0, 0.0, 1.0]  # the camera sits on the point
    assert c[2].tolist() == [-1.0, -0.0, -0.0]
    c = NR.orient_to_camera(N, P, (1.0, 1.0, 3.0))
    assert c[0].tolist() == [0.0, 0.0, 1.0] and c[1].tolist() == [-0.0, -0.6, 0.8]
    u = NR.normalize(N)
    assert u[0].tolist() == [0.0, 0.0, 0.0] and u[3].tolist() == [0.0, 0.0, 1.0]


# ------------------------------------------------------------------------------------------------ the interface
def test_search_param_classes(pkg):
    g = pkg.geometry
    assert g.KDTreeSearchParamKNN().knn == 30 and g.KDTreeSearchParamKNN(7).knn == 7
    h = g.KDTreeSearchParamHybrid(radius=0.1, max_nn=12)
    assert (h.radius, h.max_nn) == (0.1, 12)
    assert g.KDTreeSearchParamRadius(0.25).radius == 0.25
    for p in (g.KDTreeSearchParamKNN(), h, g.KDTreeSearchParamRadius(1.0)):
        assert isinstance(p, g.KDTreeSearchParam) and "KDTreeSearchParam" in repr(p)


def _cloud(pkg, n=4):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.arange(3.0 * n).reshape(n, 3))
    return p


def test_refusals_need_no_device(pkg):
    g = pkg.geometry
    for n in (4, 0):
        p = _cloud(pkg, n)
        for call in (p.estimate_normals, p.estimate_covariances,
                     lambda sp: g.PointCloud.estimate_point_covariances(p, sp)):
            with pytest.raises(RuntimeError, match="KDTreeSearchParamHybrid"):
                call(g.KDTreeSearchParamRadius(0.1))
            for k in (0, -1, 65, 1000):
                with pytest.raises(RuntimeError, match=r"1\.\.64"):
                    call(g.KDTreeSearchParamKNN(k))
                with pytest.raises(RuntimeError, match=r"1\.\.64"):
                    call(g.KDTreeSearchParamHybrid(0.1, k))
            for r in (0.0, -1.0, float("nan")):
                with pytest.raises(RuntimeError, match="radius > 0"):
                    call(g.KDTreeSearchParamHybrid(r, 30))
            with pytest.raises(RuntimeError, match="search_param"):
                call(30)
        with pytest.raises(RuntimeError, match="fast_normal_computation=False"):
            p.estimate_normals(g.KDTreeSearchParamKNN(), fast_normal_computation=False)
        with pytest.raises(RuntimeError, match="fast_normal_computation=False"):
            p.estimate_normals(fast_normal_computation=False)
        assert not p.has_normals() and not p.has_covariances()
        for call in (p.orient_normals_to_align_with_direction, p.orient_normals_towards_camera_location):
            with pytest.raises(RuntimeError, match="No normals in the PointCloud"):
                call()


def test_empty_cloud_is_a_no_op(pkg):
    g = pkg.geometry
    p = g.PointCloud()
    assert p.estimate_normals() is None and p.estimate_covariances(g.KDTreeSearchParamHybrid(0.1, 5)) is None
    assert not p.has_normals() and not p.has_covariances()
    assert len(p.covariances) == 0 and np.asarray(p.covariances).shape == (0, 3, 3)
    assert len(g.PointCloud.estimate_point_covariances(p, g.KDTreeSearchParamKNN())) == 0
    assert p.normalize_normals() is p


def test_covariances_property_is_a_host_view(pkg):
    p = _cloud(pkg, 2)
    cov = np.arange(18.0).reshape(2, 3, 3)
    p.covariances = cov
    assert p.has_covariances()
    v = p.covariances
    assert len(v) == 2 and np.asarray(v).shape == (2, 3, 3)
    assert_bitwise(np.asarray(v), cov, "covariances round trip")
    np.asarray(v)[1, 2, 2] = -1.0  # a view, as the other vectors
    assert np.asarray(p.covariances)[1, 2, 2] == -1.0
    cov[0, 0, 0] = 99.0  # the setter copied
    assert np.asarray(p.covariances)[0, 0, 0] == 0.0
    p.points = pkg.utility.Vector3dVector(np.zeros((3, 3)))
    assert not p.has_covariances()  # as many matrices as points, or none


def test_header_declares_and_table_binds_the_calls(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.native_library()
    for name, nargs in (("ot_estimate_covariances", 6), ("ot_estimate_normals", 8), ("ot_orient_normals", 6),
                        ("ot_normalize_normals", 3)):
        assert re.search(r"\bot_status\s+" + name + r"\s*\(", src)
        assert len(pkg._lib.SIGNATURES[name]) == nargs
        assert name not in lib._ot_missing
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "estimate_normals" in text and "ot_estimate_normals" in text


@pytest.mark.parametrize("knn,radius", [(0, 0.0), (65, 0.0), (-3, 0.1), (30, float("nan"))])
def test_c_abi_argument_errors_need_no_device(pkg, knn, radius):
    lib = pkg.native_library()
    pts = np.zeros((4, 3))
    out = np.zeros((4, 9))
    nrm = np.zeros((4, 3))
    st = lib.ot_estimate_covariances(pts.ctypes.data_as(C.c_void_p), 4, knn, radius, out.ctypes.data_as(C.c_void_p),
                                     None)
    assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert lib.ot_last_error().decode().startswith("[EstimateCovariances]")
    st = lib.ot_estimate_normals(pts.ctypes.data_as(C.c_void_p), 4, knn, radius, None,
                                 nrm.ctypes.data_as(C.c_void_p), None, None)
    assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert lib.ot_last_error().decode().startswith("[EstimateNormals]")


def test_c_abi_empty_and_bad_mode(pkg):
    lib = pkg.native_library()
    ref = (C.c_double * 3)(0.0, 0.0, 1.0)
    assert lib.ot_estimate_covariances(None, 0, 30, 0.0, None, None) == pkg._lib.OT_OK
    assert lib.ot_estimate_normals(None, 0, 30, 0.0, None, None, None, None) == pkg._lib.OT_OK
    assert lib.ot_orient_normals(None, None, 0, 0, ref, None) == pkg._lib.OT_OK
    assert lib.ot_normalize_normals(None, 0, None) == pkg._lib.OT_OK
    assert lib.ot_orient_normals(None, None, 4, 2, ref, None) == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert lib.ot_last_error().decode().startswith("[OrientNormals]")
