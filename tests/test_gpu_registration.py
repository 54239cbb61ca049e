"""GPU parity: PointCloud.transform / rotate / translate / get_center / deepcopy and pipelines.registration
(evaluate_registration, registration_icp) against the numpy restatement in icp_ref.py ("registration").

The scene (icp_ref.scene) is analytic and seeded: 4,800 target points, 2,800 source points of which 300 have no
correspondence.  The reference ICP is computed once per angle and shared.  Tolerances: correspondences, fitness and
every matched d2 are compared exactly (the same float64 operations in the same order); inlier_rmse and the
transformation depend on a summation order and an SVD and get the bounds reasoned in each test."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_ref as R
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu

T_NONTRIVIAL = np.array([[0.9362933635841992, -0.2896294776255156, 0.1986693307950612, 0.37],
                         [0.3129918003881019, 0.9447025165397181, -0.0978433950072557, -1.25],
                         [-0.1593450969499678, 0.1537920558182814, 0.9751703272018158, 2.5],
                         [0.0, 0.0, 0.0, 1.0]])


def _pcd(pkg, xyz, normals=None):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(xyz)
    if normals is not None:
        p.normals = pkg.utility.Vector3dVector(normals)
    return p


def _last_d2(pkg, n):
    """the per-source-point d2 of the last evaluation (test hook; -1: no correspondence)"""
    import torch

    out = torch.empty(n, dtype=torch.float64, device="cuda")
    pkg._lib.call("otx_registration_last_d2", C.c_void_p(out.data_ptr()), n, None)
    return out.cpu().numpy()


def _check_evaluation(pkg, res, ref, n, what):
    """correspondences, fitness and the matched d2 exactly; rmse to 1e-12 relative (another summation order)"""
    assert_bitwise(np.asarray(res.correspondence_set), ref.corr, what + ": correspondence_set")
    assert np.asarray(res.correspondence_set).dtype == np.int32
    assert_bitwise(np.float64(res.fitness), np.float64(ref.fitness), what + ": fitness")
    assert abs(res.inlier_rmse - ref.inlier_rmse) <= 1e-12 * ref.inlier_rmse, (what, res.inlier_rmse, ref.inlier_rmse)
    if n and ref.corr.shape[0]:
        d2 = _last_d2(pkg, n)
        ok = ref.idx >= 0
        assert_bitwise(d2[ok], ref.d2[ok], what + ": matched d2")
        assert np.all(d2[~ok] == -1.0)


# ------------------------------------------------------------------------------------------- 1. the motion API
def test_transform_rotate_translate_bitwise(pkg, gpu):
    src, _, _ = R.scene(1)
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=src.shape)
    p = _pcd(pkg, src, nrm)
    assert p.transform(T_NONTRIVIAL) is p
    assert_bitwise(np.asarray(p.points), R.transform_points(src, T_NONTRIVIAL), "transform: points")
    assert_bitwise(np.asarray(p.normals), R.transform_normals(nrm, T_NONTRIVIAL), "transform: normals")
    # a projective last row exercises the division by w'
    Tp = T_NONTRIVIAL.copy()
    Tp[3] = [0.01, -0.02, 0.005, 1.1]
    q = _pcd(pkg, src).transform(Tp)
    assert_bitwise(np.asarray(q.points), R.transform_points(src, Tp), "transform: projective")

    Rm = pkg.geometry.get_rotation_matrix_from_xyz((0.2, -0.4, 1.3))
    for center in ((0, 0, 0), (-4.0, 5.0, 0.5)):
        p = _pcd(pkg, src, nrm)
        assert p.rotate(Rm, center=center) is p
        Tr = R.rotate_matrix(Rm, np.asarray(center, np.float64))
        assert_bitwise(np.asarray(p.points), R.transform_points(src, Tr), f"rotate about {center}: points")
        assert_bitwise(np.asarray(p.normals), R.transform_normals(nrm, Tr), f"rotate about {center}: normals")
    # the reference's call (center at the origin) is exactly R p
    Rp = np.stack([(Rm[r, 0] * src[:, 0] + Rm[r, 1] * src[:, 1]) + Rm[r, 2] * src[:, 2] for r in range(3)], axis=1)
    assert np.array_equal(np.asarray(_pcd(pkg, src).rotate(Rm, center=(0, 0, 0)).points), Rp)
    # default centre: get_center()
    p = _pcd(pkg, src)
    c = p.get_center()
    p.rotate(Rm)
    assert_bitwise(np.asarray(p.points), R.transform_points(src, R.rotate_matrix(Rm, c)), "rotate about the centre")

    t = np.array([-1.0, 0.25, 3.5])
    p = _pcd(pkg, src, nrm)
    assert p.translate(t) is p
    assert_bitwise(np.asarray(p.points), src + t, "translate")
    assert_bitwise(np.asarray(p.normals), nrm, "translate keeps normals")
    p = _pcd(pkg, src)
    c = p.get_center()
    p.translate(t, relative=False)
    assert_bitwise(np.asarray(p.points), src + (t - c), "translate(relative=False)")


def test_get_center_and_deepcopy(pkg, gpu):
    src, _, _ = R.scene(1)
    seq = np.zeros(3)
    for row in src:
        seq += row
    seq /= src.shape[0]
    p = _pcd(pkg, src)
    assert np.abs(p.get_center() - seq).max() <= 1e-12
    p.transform(np.eye(4))  # now device resident
    assert np.abs(p.get_center() - seq).max() <= 1e-12
    assert np.array_equal(pkg.geometry.PointCloud().get_center(), np.zeros(3))

    q = copy.deepcopy(p)
    q.translate([1.0, 2.0, 3.0])
    assert_bitwise(np.asarray(p.points), src, "deepcopy: the original is untouched")
    assert_bitwise(np.asarray(q.points), src + np.array([1.0, 2.0, 3.0]), "deepcopy: the copy moved")
    h = _pcd(pkg, src)  # host-resident original
    g = copy.deepcopy(h)
    np.asarray(g.points)[0, 0] = 99.0
    assert np.asarray(h.points)[0, 0] == src[0, 0]


# ---------------------------------------------------------------------- 2. one evaluation, identity and other init
@pytest.mark.parametrize("init", ["identity", "moved"])
def test_evaluate_and_zero_iteration_icp(pkg, gpu, init):
    reg = pkg.pipelines.registration
    src, tgt, T_gt = R.scene(1)
    T = np.eye(4) if init == "identity" else T_gt
    ref = R.evaluate(R.transform_points(src, T), tgt, R.R_CORR)
    assert 0 < ref.corr.shape[0] < src.shape[0]
    res = reg.evaluate_registration(_pcd(pkg, src), _pcd(pkg, tgt), R.R_CORR, T)
    _check_evaluation(pkg, res, ref, src.shape[0], f"evaluate_registration ({init})")
    assert_bitwise(res.transformation, T, "evaluate: transformation")
    if init == "identity":  # ICP does not transform by an identity init (the same points either way)
        ref = R.evaluate(src, tgt, R.R_CORR)
    res = reg.registration_icp(_pcd(pkg, src), _pcd(pkg, tgt), R.R_CORR, T,
                               reg.TransformationEstimationPointToPoint(),
                               reg.ICPConvergenceCriteria(max_iteration=0))
    _check_evaluation(pkg, res, ref, src.shape[0], f"registration_icp(max_iteration=0) ({init})")
    assert_bitwise(res.transformation, T, "icp(0): transformation = init")
    assert res.iterations == 0


def test_exact_ties_go_to_the_lowest_index(pkg, gpu):
    reg = pkg.pipelines.registration
    src, tgt, _ = R.scene(1)
    rng = np.random.default_rng(5)
    perm = rng.permutation(tgt.shape[0])
    dup = np.concatenate([tgt[perm], tgt, tgt[perm[:1000]]])  # every target point two or three times
    ref = R.evaluate(src, dup, R.R_CORR)
    res = reg.evaluate_registration(_pcd(pkg, src), _pcd(pkg, dup), R.R_CORR, np.eye(4))
    _check_evaluation(pkg, res, ref, src.shape[0], "duplicated targets")
    # the matched source points themselves as targets: d2 = 0 ties between copies
    self_t = np.concatenate([src[:700], src[:700]])
    ref = R.evaluate(src, self_t, R.R_CORR)
    res = reg.evaluate_registration(_pcd(pkg, src), _pcd(pkg, self_t), R.R_CORR, np.eye(4))
    _check_evaluation(pkg, res, ref, src.shape[0], "zero-distance ties")
    assert np.all(np.asarray(res.correspondence_set)[:700, 1] == np.arange(700))


def test_degenerate_inputs(pkg, gpu):
    reg = pkg.pipelines.registration
    src, tgt, _ = R.scene(1)
    one = tgt[1234:1235]
    ref = R.evaluate(src, one, R.R_CORR)
    res = reg.evaluate_registration(_pcd(pkg, src), _pcd(pkg, one), R.R_CORR, np.eye(4))
    _check_evaluation(pkg, res, ref, src.shape[0], "one-point target")
    crit = reg.ICPConvergenceCriteria(max_iteration=5)
    for s, t in ((src, np.zeros((0, 3))), (np.zeros((0, 3)), tgt)):
        for res in (reg.evaluate_registration(_pcd(pkg, s), _pcd(pkg, t), R.R_CORR, T_NONTRIVIAL),
                    reg.registration_icp(_pcd(pkg, s), _pcd(pkg, t), R.R_CORR, T_NONTRIVIAL,
                                         reg.TransformationEstimationPointToPoint(), crit)):
            assert (res.fitness, res.inlier_rmse, res.iterations) == (0.0, 0.0, 0)
            assert np.asarray(res.correspondence_set).shape == (0, 2)
            assert_bitwise(res.transformation, T_NONTRIVIAL, "empty cloud: T = init")
    for r in (0.0, -0.05):
        with pytest.raises(RuntimeError, match=r"^Invalid max_correspondence_distance\.$"):
            reg.registration_icp(_pcd(pkg, src), _pcd(pkg, tgt), r, np.eye(4))


# --------------------------------------------------------------------------------- 3. per-iteration parity
@pytest.mark.parametrize("max_iteration", [1, 2, 3])
def test_per_iteration_parity(pkg, gpu, max_iteration):
    reg = pkg.pipelines.registration
    src, tgt, _ = R.scene(3)
    ref = R.reference_icp(3, max_iteration)
    # preconditions on the reference's own trajectory: no near tie and no d2 near the radius, so roundoff in the
    # accumulated transformation (1e-15 m on coordinates, 1e-16 m^2 on d2) cannot change a pair
    assert ref.min_gap >= 1e-10, ref.min_gap
    assert ref.min_margin >= 1e-6, ref.min_margin
    assert ref.iterations == max_iteration
    res = reg.registration_icp(_pcd(pkg, src), _pcd(pkg, tgt), R.R_CORR, np.eye(4),
                               reg.TransformationEstimationPointToPoint(),
                               reg.ICPConvergenceCriteria(max_iteration=max_iteration))
    assert res.iterations == max_iteration
    assert_bitwise(np.asarray(res.correspondence_set), ref.corr, "correspondence_set")
    assert_bitwise(np.float64(res.fitness), np.float64(ref.fitness), "fitness")
    assert abs(res.inlier_rmse - ref.inlier_rmse) <= 1e-9 * ref.inlier_rmse, (res.inlier_rmse, ref.inlier_rmse)
    assert np.abs(res.transformation - ref.transformation).max() <= 1e-10


# ------------------------------------------------------------------------------------------ 4. convergence
@pytest.mark.parametrize("deg,max_iteration", [(1, 30), (3, 30), (3, 2000)])
def test_convergence_to_the_known_transformation(pkg, gpu, deg, max_iteration):
    reg = pkg.pipelines.registration
    src, tgt, T_gt = R.scene(deg)
    ref = R.reference_icp(deg)
    assert ref.min_gap >= 1e-10 and ref.min_margin >= 1e-6
    res = reg.registration_icp(_pcd(pkg, src), _pcd(pkg, tgt), 0.05, np.eye(4),
                               reg.TransformationEstimationPointToPoint(),
                               reg.ICPConvergenceCriteria(max_iteration=max_iteration))
    assert res.iterations == ref.iterations
    assert res.fitness == 2500 / 2800
    assert res.inlier_rmse < 1e-10
    assert np.abs(res.transformation - T_gt).max() <= 1e-10
    assert_bitwise(np.asarray(res.correspondence_set), ref.corr, "correspondence_set")


# ------------------------------------------------------------------------------------------ 5. determinism
def test_two_calls_give_the_same_bits(pkg, gpu):
    reg = pkg.pipelines.registration
    src, tgt, _ = R.scene(3)
    runs = [reg.registration_icp(_pcd(pkg, src), _pcd(pkg, tgt), R.R_CORR, np.eye(4),
                                 reg.TransformationEstimationPointToPoint(), reg.ICPConvergenceCriteria())
            for _ in range(2)]
    assert_bitwise(runs[0].transformation, runs[1].transformation, "transformation")
    assert_bitwise(np.float64(runs[0].inlier_rmse), np.float64(runs[1].inlier_rmse), "inlier_rmse")
    assert_bitwise(np.asarray(runs[0].correspondence_set), np.asarray(runs[1].correspondence_set), "pairs")
    assert runs[0].iterations == runs[1].iterations


# --------------------------------------------------------------------------- 6. a surface-like cloud from synth
def test_surface_clouds_against_exhaustive_search(pkg, O, synth, seq16, gpu):
    depth, color, ext = seq16
    intr = ref_intr(synth)
    clouds = []
    for f in (0, 1):
        xyz = O.unproject(O.depth_to_float(depth[f], 1000.0, 5.0), color[f], intr, ext[f])[0]
        for voxel in (0.02, 0.03, 0.04, 0.06, 0.08, 0.12):
            down = O.voxel_down_sample(xyz, None, voxel)[0]
            if down.shape[0] <= 6000:
                break
        assert 500 < down.shape[0] <= 6000
        clouds.append(down)
    a, b = clouds
    ref = R.evaluate(a, b, R.R_CORR)
    assert 0 < ref.corr.shape[0] < a.shape[0]  # both matched and unmatched queries
    res = pkg.pipelines.registration.evaluate_registration(_pcd(pkg, a), _pcd(pkg, b), R.R_CORR, np.eye(4))
    _check_evaluation(pkg, res, ref, a.shape[0], "surface clouds")
    d = O.point_cloud_distance(a, b)
    d2 = _last_d2(pkg, a.shape[0])
    near = d * d < R.R_CORR * R.R_CORR * (1 - 1e-12)
    assert_bitwise(np.sqrt(d2[near]), d[near], "d2 against the oracle's 1-NN distances")


# ------------------------------------------------------------------------------------- 7. the restated caller
def test_refine_icp_moves_the_source_by_the_result(pkg, gpu):
    ev = importlib.import_module(pkg.__name__ + ".evaluation")
    src, tgt, T_gt = R.scene(1)
    reg = pkg.pipelines.registration.registration_icp(
        _pcd(pkg, src), _pcd(pkg, tgt), 0.05, np.eye(4),
        pkg.pipelines.registration.TransformationEstimationPointToPoint(),
        pkg.pipelines.registration.ICPConvergenceCriteria(max_iteration=2000))
    source = _pcd(pkg, src)
    out = ev.refine_icp(source, _pcd(pkg, tgt))
    assert out is source
    assert_bitwise(np.asarray(out.points), R.transform_points(src, reg.transformation), "refined source")
    assert np.abs(reg.transformation - T_gt).max() <= 1e-10
    moved = ev.apply_transform(_pcd(pkg, src), [10.0, -20.0, 30.0], [-4.5, 5.6, 0.0])
    Rm = pkg.geometry.get_rotation_matrix_from_xyz(tuple(np.radians([10.0, -20.0, 30.0])))
    exp = R.transform_points(src, R.rotate_matrix(Rm, np.zeros(3))) + np.array([-4.5, 5.6, 0.0])
    assert_bitwise(np.asarray(moved.points), exp, "apply_transform")
    acc, comp = ev.calculate_metrics(out, _pcd(pkg, tgt))
    assert acc >= 0.0 and comp >= 0.0
