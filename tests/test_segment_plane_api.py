"""PointCloud.segment_plane without a device: the numpy reference (tests/segment_plane_ref.py) states the serial loop
and the closed form the GPU computes; here the two agree bit for bit, known answers hold, the argument errors come in
order, the C ABI is declared and bound, and the designed clouds (tests/segment_plane_clouds.py) have the properties
test_gpu_segment_plane.py relies on -- asserted on the reference alone, so no GPU test passes vacuously."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import segment_plane_clouds as SC
import segment_plane_ref as SP
from conftest import ROOT, assert_bitwise


def _both(pts, thr, rn=3, iters=100, prob=0.99999999, seed=0, what=""):
    a = SP.segment_plane_loop(pts, thr, rn, iters, prob, seed)
    b = SP.segment_plane(pts, thr, rn, iters, prob, seed)
    assert_bitwise(b.plane, a.plane, f"{what}: plane, closed form vs loop")
    assert_bitwise(b.inliers, a.inliers, f"{what}: inliers, closed form vs loop")
    assert (b.evaluated, b.skipped, b.margin, b.broke) == (a.evaluated, a.skipped, a.margin, a.broke), what
    return a


@pytest.fixture(scope="module")
def designed():
    """name -> Result of the loop (checked against the closed form) for every designed case"""
    out = {}
    for name, pts, thr, rn, iters, prob, seed in SC.random_cases() + SC.long_run_cases():
        out[name] = _both(pts, thr, rn, iters, prob, seed, name)
    for name, pts, thr, rn in SC.size_cases():
        out[name] = _both(pts, thr, rn, 100, what=name)
    out["slabs exact+jittered"] = [_both(SC.slabs_exact_and_jittered(), SC.SLAB_THRESHOLD, seed=s,
                                         what=f"slabs exact+jittered, seed {s}") for s in range(4)]
    out["slabs both exact"] = [_both(SC.slabs_both_exact(), SC.SLAB_THRESHOLD, seed=s,
                                     what=f"slabs both exact, seed {s}") for s in range(4)]
    pts, _ = SC.at_threshold()
    out["threshold 0.25"] = _both(pts, 0.25, what="threshold 0.25")
    out["threshold 0.25+"] = _both(pts, np.nextafter(0.25, 1.0), what="threshold nextafter(0.25)")
    out["degenerate"] = _both(SC.degenerate(), 0.01, iters=200, what="degenerate")
    out["one plane"] = _both(SC.one_plane(), 0.01, what="one plane")
    out["offset"] = _both(SC.offset_cloud(), SC.THRESHOLD, what="offset")
    return out


def _flat(designed):
    for v in designed.values():
        yield from (v if isinstance(v, list) else [v])


def test_loop_and_closed_form_agree_on_designed_clouds(designed):
    assert len(list(_flat(designed))) >= 25


def test_loop_and_closed_form_agree_on_random_clouds():
    """>= 50 random plane-plus-noise clouds of 1 000 - 4 096 points with 30 - 90 % plane points, 100 - 1 000 iterations.
    The figures of the run are printed; the one asserted is the margin the GPU tests rely on."""
    rng = np.random.default_rng(2024)
    margins, evaluated, ties = [], [], []
    for j in range(52):
        n = int(rng.integers(1000, 4097))
        frac = float(rng.uniform(0.3, 0.9))
        iters = int(rng.choice([100, 300, 1000]))
        rn = int(rng.choice([3, 3, 3, 4, 5]))
        r = _both(SC.plane_and_noise(1000 + j, n, frac), SC.THRESHOLD, rn, iters, seed=j,
                  what=f"random cloud {j} (n={n}, frac={frac:.2f}, ransac_n={rn}, iters={iters})")
        margins.append(r.margin)
        evaluated.append((r.evaluated, iters))
        ties.append(r.ties)
    print(f"margins: min {min(margins):.3g}; evaluated/iterations: {evaluated}; count ties: {sorted(set(ties))}")
    assert min(margins) >= 1e-6


def test_known_answers_on_integer_lattices():
    # every point on z = 2: the first non-degenerate sample gives (0, 0, +-1, -+2), all points are inliers, and the
    # refit over the lattice is exactly (0, 0, 1, -2) (xz = yz = zz = 0, det_z = xx yy - xy xy > 0)
    pts = SC.one_plane()
    r = SP.segment_plane_loop(pts, 0.01)
    assert_bitwise(r.plane, np.array([0.0, 0.0, 1.0, -2.0]), "lattice z = 2")
    assert r.inliers.tolist() == list(range(len(pts))) and r.evaluated == 1 and r.broke
    # triangle plane of three lattice points, by hand: e0 = (2, 0, 0), e1 = (0, 3, 0) -> (0, 0, 6) / 6, d = -5
    assert_bitwise(SP.triangle_plane([1.0, 1.0, 5.0], [3.0, 1.0, 5.0], [1.0, 4.0, 5.0]),
                   np.array([0.0, 0.0, 1.0, -5.0]), "triangle plane")
    assert SP.is_zero(SP.triangle_plane([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]))
    # x = 3 (det_x largest) and y = -1 (det_y largest) through GetPlaneFromPoints
    g = SC.lattice(5, 4)
    assert_bitwise(SP.plane_from_points(g[:, [2, 0, 1]] + [3.0, 0.0, 0.0], np.arange(20)),
                   np.array([1.0, 0.0, 0.0, -3.0]), "plane x = 3")
    assert_bitwise(SP.plane_from_points(g[:, [0, 2, 1]] + [0.0, -1.0, 0.0], np.arange(20)),
                   np.array([0.0, 1.0, 0.0, 1.0]), "plane y = -1")
    # collinear points span no plane; no points at all leave every moment 0, so the norm is 0 as well
    line = np.arange(5.0)[:, None] * np.array([[1.0, 2.0, 3.0]])
    assert SP.is_zero(SP.plane_from_points(line, np.arange(5)))
    assert_bitwise(SP.plane_from_points(g, []), np.zeros(4), "no points")
    # the sampler: the words of csrc/rng.h (splitmix64), distinct indices in draw order
    assert SP.rng_word(0, 0) == 0xE220A8397B1DCDAF  # splitmix64's first output for seed 0
    for it in range(50):
        s = SP.sample(5, it, 4, 4)
        assert sorted(s) == [0, 1, 2, 3]


def test_edge_values_on_the_reference():
    pts = SC.plane_and_noise(77, 500, 0.6)
    for kw in (dict(distance_threshold=0.0), dict(distance_threshold=SC.THRESHOLD, num_iterations=0)):
        for f in (SP.segment_plane_loop, SP.segment_plane):
            r = f(pts, **kw)
            # GetPlaneFromPoints over no points: the centroid is 0 / 0 but every moment sum is empty, so abc and its
            # norm are 0 and the "norm == 0" branch returns the zero plane before the centroid is used
            assert len(r.inliers) == 0
            assert_bitwise(r.plane, np.zeros(4), f"{kw}")
    r = _both(pts, SC.THRESHOLD, 3, 100, 1.0, 0, "probability 1")
    assert r.evaluated + r.skipped == 100 and not r.broke


def test_designed_clouds_have_their_properties(designed):
    flat = list(_flat(designed))
    assert any(r.broke for r in flat) and any(not r.broke and r.evaluated + r.skipped >= 100 for r in flat)
    assert sum(r.rmse_decided for r in flat) >= 1
    assert min(r.margin for r in flat) >= 1e-6
    # chunked replay: a run that breaks past the first chunk of 256, and one that runs 1000 iterations out
    assert any(r.broke and r.evaluated > 256 for r in flat) or any(r.evaluated > 512 for r in flat)
    # equal-count slabs: rmse decides at least once over the seeds and the exact slab (z = 0) always wins
    sl = designed["slabs exact+jittered"]
    assert sum(r.rmse_decided for r in sl) >= 1 and all(r.ties >= 1 for r in sl)
    pts = SC.slabs_exact_and_jittered()
    for r in sl:
        assert len(r.inliers) == 144 and (pts[r.inliers, 2] == 0.0).all()
    ex = designed["slabs both exact"]
    assert all(r.ties >= 1 and r.rmse_decided == 0 and len(r.inliers) == 144 for r in ex)
    assert len({float(SC.slabs_both_exact()[r.inliers[0], 2]) for r in ex}) == 2  # either slab can come first
    # exactly at the threshold: excluded at 0.25, included one ulp above
    pts, raised = SC.at_threshold()
    lo, hi = designed["threshold 0.25"], designed["threshold 0.25+"]
    assert len(raised) == 32 and not set(raised) & set(lo.inliers.tolist()) and len(lo.inliers) == 400
    assert set(raised) <= set(hi.inliers.tolist()) and len(hi.inliers) == 432
    assert designed["degenerate"].skipped >= 20
    one = designed["one plane"]
    assert one.evaluated == 1 and one.broke and len(one.inliers) == 500
    assert len(designed["N=4097"].inliers) > 2 * 256 and designed["N=3"].inliers.tolist() == [0, 1, 2]


def test_facade_signature_and_errors_without_a_device(pkg):
    PC = pkg.geometry.PointCloud
    assert list(inspect.signature(PC.segment_plane).parameters) == [
        "self", "distance_threshold", "ransac_n", "num_iterations", "probability", "seed"]
    d = {k: v.default for k, v in inspect.signature(PC.segment_plane).parameters.items()}
    assert (d["ransac_n"], d["num_iterations"], d["probability"], d["seed"]) == (3, 100, 0.99999999, 0)
    p = PC()
    p.points = pkg.utility.Vector3dVector(np.zeros((2, 3)))
    # in order: probability first, then ransac_n, then the point count
    for prob in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"^Probability must be > 0 and <= 1\.0$"):
            p.segment_plane(0.01, ransac_n=2, probability=prob)
    with pytest.raises(RuntimeError, match=r"^ransac_n should be set to higher than or equal to 3\.$"):
        p.segment_plane(0.01, ransac_n=2)
    with pytest.raises(RuntimeError, match=r"^There must be at least 'ransac_n' points\.$"):
        p.segment_plane(0.01)
    with pytest.raises(RuntimeError, match=r"^There must be at least 'ransac_n' points\.$"):
        PC().segment_plane(0.01, ransac_n=40)
    big = PC()
    big.points = pkg.utility.Vector3dVector(np.zeros((40, 3)))
    with pytest.raises(RuntimeError, match="ransac_n > 32 is not supported by this build"):
        big.segment_plane(0.01, ransac_n=33)
    # the reference refuses the same arguments with the same words
    for args, msg in (((2, 1.5), "Probability"), ((2, 0.5), "ransac_n should"), ((3, 0.5), "at least 'ransac_n'")):
        for f in (SP.segment_plane_loop, SP.segment_plane):
            with pytest.raises(RuntimeError, match=msg):
                f(np.zeros((2, 3)), 0.01, args[0], 100, args[1])


def test_header_declares_and_table_binds_segment_plane(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bot_status\s+ot_segment_plane\s*\(", src)
    assert len(pkg._lib.SIGNATURES["ot_segment_plane"]) == 12
    lib = pkg.native_library()
    assert "ot_segment_plane" not in lib._ot_missing
    assert lib.ot_abi_version() == 1


def test_c_abi_argument_errors_without_a_device(pkg):
    lib = pkg.native_library()
    pts = np.zeros((40, 3))
    plane, k, ev = np.zeros(4), C.c_int64(-1), C.c_int32(-1)

    def call(n, rn, prob):
        return lib.ot_segment_plane(pts.ctypes.data_as(C.c_void_p), n, 0.01, rn, 100, prob, 0,
                                    plane.ctypes.data_as(C.c_void_p), None, C.byref(k), C.byref(ev), None)

    for (n, rn, prob), msg in (((2, 2, 0.0), b"Probability must be > 0 and <= 1.0"),
                               ((2, 2, 2.0), b"Probability must be > 0 and <= 1.0"),
                               ((2, 2, 0.5), b"ransac_n should be set to higher than or equal to 3."),
                               ((2, 3, 0.5), b"There must be at least 'ransac_n' points."),
                               ((40, 33, 0.5), b"ransac_n > 32 is not supported by this build")):
        assert call(n, rn, prob) == pkg._lib.OT_ERR_INVALID_ARGUMENT
        assert msg in lib.ot_last_error()
    assert k.value == -1 and ev.value == -1


def test_break_threshold_follows_the_definition():
    m = []
    assert SP.break_iteration(1.0, 3, 0.99, 100, m) == 0
    assert SP.break_iteration(0.5, 3, 1.0, 100, m) == 100        # log(0): not finite
    assert SP.break_iteration(1e-6, 3, 0.99, 100, m) == 100      # fitness^3 below 2^-53: log(1) = 0
    assert SP.break_iteration(0.5, 3, 0.99999999, 1000, m) == \
        math.trunc(math.log(1.0 - 0.99999999) / math.log(0.875)) == 137
    assert SP.break_iteration(0.5, 3, 0.99999999, 100, m) == 100
    assert SP.break_iteration(0.9, 3, 1e-300, 100, m) == 0       # log(1 - tiny) = 0, quotient -0.0: finite and >= 0
