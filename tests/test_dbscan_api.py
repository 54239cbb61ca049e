"""PointCloud.cluster_dbscan without a device: the numpy reference (tests/dbscan_ref.py) states Open3D's loop and the
closed form the GPU computes, and they agree on random clouds and on every designed cloud of test_gpu_dbscan.py,
whose properties are asserted here; known lattice answers; the C ABI declaration and binding; argument errors, which
are raised before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dbscan_clouds as DC
import dbscan_ref as DB
from conftest import ROOT, assert_bitwise


def _agree(pts, eps, mp, what):
    loop, closed, core, nbs = DB.both(pts, eps, mp)
    assert loop.dtype == closed.dtype == np.int32
    assert_bitwise(loop, closed, f"{what}: Open3D's loop vs the closed form")
    assert (loop >= -1).all()
    return closed, core, nbs


def test_loop_and_closed_form_agree_on_random_clouds():
    cases = DC.random_cases(3)
    assert len(cases) >= 50
    seen_noise = seen_border = seen_multi = 0
    for pts, eps, mp in cases:
        assert len(pts) <= 500
        lab, core, _ = _agree(pts, eps, mp, f"blobs, eps = {eps}, min_points = {mp}")
        seen_noise += int((lab == -1).any())
        seen_border += int((~core & (lab >= 0)).any())
        seen_multi += int(lab.max() >= 1)
        perm = np.random.default_rng(len(pts)).permutation(len(pts))
        _agree(pts[perm], eps, mp, "the same cloud permuted")
    assert seen_noise > 10 and seen_border > 10 and seen_multi > 10  # the sweep exercises every kind of point


def test_lattice_known_answers():
    e = DC.LATTICE_EPS
    up = float(np.nextafter(e, 1.0))
    pts = DC.lattice() * e
    assert pts.shape == (120, 3)
    lab, core, _ = _agree(pts, e, 1, "lattice at exactly eps, min_points = 1")
    assert lab.tolist() == list(range(120))  # neighbours at exactly eps are excluded by the strict <
    lab, core, _ = _agree(pts, e, 2, "lattice at exactly eps, min_points = 2")
    assert (lab == -1).all()
    for mp, n_core, n_noise in ((4, 120, 0), (5, 112, 0), (7, 24, 44), (8, 0, 120)):
        lab, core, _ = _agree(pts, up, mp, f"lattice, eps one double above the spacing, min_points = {mp}")
        assert int(core.sum()) == n_core and int((lab == -1).sum()) == n_noise
        assert set(lab.tolist()) <= {-1, 0}
        if n_core:
            assert (lab[core] == 0).all()
    for name, p, eps, mp in DC.lattice_cases():
        _agree(p, eps, mp, f"lattice {name}, min_points = {mp}")


def test_contested_border_points_take_the_lower_cluster():
    pts, eps, mp, single = DC.contested()
    assert len(pts) <= 5000
    lab, core, nbs = _agree(pts, eps, mp, "contested border points")
    assert lab.max() == 1
    contested = 0
    for i in single:
        assert not core[i]
        cn = nbs[i][core[nbs[i]]]
        d = np.linalg.norm(pts[cn] - pts[i], axis=1)
        if set(lab[cn].tolist()) == {0, 1} and lab[cn[np.argmin(d)]] == 1:
            contested += 1
            assert lab[i] == 0
    assert contested >= 5
    assert contested == len(single)


def test_noise_first_and_isolated_points():
    pts, eps, mp, n_fringe, n_lone = DC.noise_first()
    lab, core, nbs = _agree(pts, eps, mp, "border points stored before their cluster")
    assert not core[:n_fringe].any() and core[n_fringe:len(pts) - n_lone].all()
    assert np.nonzero(core)[0].min() > n_fringe - 1
    assert lab[:n_fringe].tolist() == np.repeat(np.arange(6), 4).tolist()  # claimed after being marked noise
    assert (lab[len(pts) - n_lone:] == -1).all()
    assert all(len(nbs[i]) == 1 for i in range(len(pts) - n_lone, len(pts)))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_straddling_pairs_are_two_point_clusters(axis):
    ran = 0
    for pts, r, k in DC.straddle_cases(axis):
        assert len(pts) <= 5000
        lab, core, _ = _agree(pts, r, 2, f"cell-straddling pairs along axis {axis} (r = {r})")
        assert lab[0] == -1
        assert lab[1:2 * k + 1].tolist() == np.repeat(np.arange(k), 2).tolist()
        ran += k
    assert ran > 2000


def test_chains_are_one_cluster():
    eps = DC.CHAIN_EPS
    pts = DC.chain(4096)
    rng = np.random.default_rng(47)
    for mp in (2, 3):
        for name, p in (("index order", pts), ("reversed", pts[::-1]), ("permuted", pts[rng.permutation(4096)])):
            lab, core, nbs = _agree(p, eps, mp, f"chain of 4096, {name}, min_points = {mp}")
            assert (lab == 0).all()
            assert int(core.sum()) == (4096 if mp == 2 else 4094)
    assert max(len(nb) for nb in nbs) == 3  # only consecutive points are neighbours
    two = DC.two_chains()
    assert len(two) <= 5000
    for mp in (2, 3):
        lab, core, _ = _agree(two, eps, mp, f"two interleaved chains, min_points = {mp}")
        assert (lab[0::2] == 0).all() and (lab[1::2] == 1).all()


def test_coincident_groups():
    pts, eps, m, sizes, gid = DC.coincident()
    lab, core, _ = _agree(pts, eps, m, "coincident groups")
    assert_bitwise(core, sizes >= m, "groups of m and m + 1 are core, groups of m - 1 are not")
    assert (lab[sizes < m] == -1).all()
    assert lab.max() + 1 == len(set(gid[sizes >= m].tolist()))
    for g in set(gid.tolist()):
        assert len(set(lab[gid == g].tolist())) == 1


def test_small_and_odd_sizes():
    for name, pts, eps, mp in DC.small_cases():
        lab, core, _ = _agree(pts, eps, mp, f"{name}, min_points = {mp}")
        if mp <= 1:
            assert core.all() and (lab >= 0).all()
        if mp > len(pts):
            assert (lab == -1).all()


def test_reference_refuses_bad_arguments():
    pts = DC.blob_cloud(1, 50)
    for eps, mp in ((0.0, 3), (float("nan"), 3), (float("inf"), 3), (-1.0, 3), (0.1, -1)):
        with pytest.raises(RuntimeError):
            DB.cluster_dbscan(pts, eps, mp)
        with pytest.raises(RuntimeError):
            DB.cluster_dbscan_loop(pts, eps, mp)


# ------------------------------------------------------------------------------------------------ the interface
def test_header_declares_and_table_binds_cluster_dbscan(pkg):
    src = open(os.path.join(ROOT, "include", "otslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bot_status\s+ot_cluster_dbscan\s*\(", src)
    assert "ot_cluster_dbscan" in pkg._lib.SIGNATURES
    assert len(pkg._lib.SIGNATURES["ot_cluster_dbscan"]) == 7
    lib = pkg.native_library()
    assert "ot_cluster_dbscan" not in lib._ot_missing


@pytest.mark.parametrize("eps,mp", [(0.0, 3), (float("nan"), 3), (0.1, -1)])
def test_c_abi_argument_errors_need_no_device(pkg, eps, mp):
    lib = pkg.native_library()
    pts = np.zeros((4, 3))
    labels = np.zeros(4, np.int32)
    k = C.c_int32(7)
    st = lib.ot_cluster_dbscan(pts.ctypes.data_as(C.c_void_p), 4, eps, mp, labels.ctypes.data_as(C.c_void_p),
                               C.byref(k), None)
    assert st == pkg._lib.OT_ERR_INVALID_ARGUMENT
    assert lib.ot_last_error().decode().startswith("[ClusterDBSCAN]")


@pytest.mark.parametrize("eps,mp", [(0.0, 3), (float("nan"), 3), (0.1, -1)])
def test_facade_argument_errors_need_no_device(pkg, eps, mp):
    p = pkg.geometry.PointCloud()
    p.points = pkg.utility.Vector3dVector(np.zeros((4, 3)))
    with pytest.raises(RuntimeError, match=r"\[ClusterDBSCAN\]"):
        p.cluster_dbscan(eps, mp)
    with pytest.raises(RuntimeError, match=r"\[ClusterDBSCAN\]"):
        p.cluster_dbscan(eps=eps, min_points=mp, print_progress=True)


def test_empty_cloud_returns_empty_int_vector(pkg):
    out = pkg.geometry.PointCloud().cluster_dbscan(0.1, 3)
    assert isinstance(out, pkg.utility.IntVector) and len(out) == 0
    lib = pkg.native_library()
    k = C.c_int32(7)
    assert lib.ot_cluster_dbscan(None, 0, 0.1, 3, None, C.byref(k), None) == pkg._lib.OT_OK
    assert k.value == 0
