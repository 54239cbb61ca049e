"""GPU parity of compute_fpfh_feature (csrc/features.hip over the neighbour lists of csrc/nb_list.h) with the
exhaustive numpy statement (tests/fpfh_ref.py): SPFH (through spfh_out) and FPFH bit for bit on every point that is
not fragile, and at most 1 % of a cloud's points may be fragile (on the designed clouds the reference flags none:
tests/test_fpfh_ref.py asserts it)."""
import numpy as np
import pytest

import fpfh_clouds as FC
import fpfh_ref as FR
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu

ALL = sorted(FC.cases())


def _run(pkg, P, N, k, radius):
    """(spfh, fpfh) [n][33] through the C ABI"""
    D, L = pkg._device, pkg._lib
    n = len(P)
    xyz, nrm = D.to_device(np.ascontiguousarray(P, np.float64)), D.to_device(np.ascontiguousarray(N, np.float64))
    S, F = D.empty((n, 33), "float64"), D.empty((n, 33), "float64")
    S.fill_(np.nan)
    F.fill_(np.nan)
    L.call("ot_compute_fpfh_feature", D.ptr(xyz), D.ptr(nrm), n, k, 0.0 if radius is None else radius, D.ptr(F),
           D.ptr(S), D.stream_ptr())
    return D.to_host(S), D.to_host(F)


def _compare(S, F, ref, what):
    sf, ff = ref["spfh_fragile"], ref["fpfh_fragile"]
    n = len(sf)
    print(f"{what}: {n} points, {int(sf.sum())} SPFH-fragile, {int(ff.sum())} FPFH-fragile")
    assert ff.sum() <= 0.01 * n and sf.sum() <= 0.01 * n
    assert_bitwise(S[~sf], ref["spfh"][~sf], f"{what} SPFH")
    assert_bitwise(F[~ff], ref["fpfh"][~ff], f"{what} FPFH")


@pytest.mark.parametrize("name", ALL)
def test_spfh_and_fpfh_bitwise(pkg, gpu, name):
    P, N, k, radius = FC.cases()[name]
    S, F = _run(pkg, P, N, k, radius)
    _compare(S, F, FC.reference(name), name)


def test_planar_cloud(pkg, gpu):
    P, N = FC.planar()
    S, F = _run(pkg, P, N, 11, None)
    _compare(S, F, FR.compute(P, N, 11), "planar")
    assert (S[:, [5, 16, 27]] == 100.0).all() and S.sum() == 300.0 * len(P)


def test_repeat_run_is_bit_identical(pkg, gpu):
    P, N, k, radius = FC.cases()["sphere_hybrid_k100"]
    a, b = _run(pkg, P, N, k, radius), _run(pkg, P, N, k, radius)
    assert_bitwise(a[0], b[0], "SPFH twice")
    assert_bitwise(a[1], b[1], "FPFH twice")


def test_python_call_and_optional_spfh(pkg, gpu):
    """the facade (no spfh_out: the library's own workspace) gives the same feature, as a (33, n) array"""
    g, r = pkg.geometry, pkg.pipelines.registration
    for name, sp in (("random_k20", g.KDTreeSearchParamKNN(20)),
                     ("sphere_hybrid_k100", g.KDTreeSearchParamHybrid(0.06, 100))):
        P, N, k, radius = FC.cases()[name]
        pcd = g.PointCloud()
        pcd.points, pcd.normals = pkg.utility.Vector3dVector(P), pkg.utility.Vector3dVector(N)
        f = r.compute_fpfh_feature(pcd, sp)
        assert isinstance(f, r.Feature) and f.dimension() == 33 and f.num() == len(P)
        assert f.data.shape == (33, len(P)) and f.data.flags["C_CONTIGUOUS"]
        _, F = _run(pkg, P, N, k, radius)
        assert_bitwise(f.data, F.T, f"{name} through the facade")


def test_device_resident_cloud_from_voxel_down_sample(pkg, synth, seq16, gpu):
    """One frame of the package's own pipeline, never downloaded before the feature is computed; the reference is fed
    the GPU's own normals.  The normals come from a search radius of 1.5 voxels: with a wide one, neighbouring points
    of a sparse patch get the same neighbour set in another order, hence normals that differ in their last bits only,
    and the swap between such a pair is a tie (the reference then flags 2 to 9 % of this cloud as fragile)."""
    depth, color, ext = (a[1] for a in seq16)
    intr = pkg.camera.PinholeCameraIntrinsic(*ref_intr(synth))
    rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(color), pkg.geometry.Image(depth), depth_scale=1000.0, depth_trunc=5.0,
        convert_rgb_to_intensity=False)
    ds = pkg.geometry.PointCloud.create_from_rgbd_image(rgbd, intr, ext).voxel_down_sample(0.1)
    ds.estimate_normals(pkg.geometry.KDTreeSearchParamHybrid(0.15, 20))
    f = pkg.pipelines.registration.compute_fpfh_feature(ds, pkg.geometry.KDTreeSearchParamHybrid(0.5, 40))
    assert ds._xyz._h is None and ds._nrm._h is None and f._h is None  # all still on the device only
    P, N = np.array(ds.points), np.array(ds.normals)
    print(f"surface cloud after voxel_down_sample(0.1): {len(P)} points")
    assert 100 < len(P) <= 5000
    ref = FR.compute(P, N, 40, 0.5)
    ff = ref["fpfh_fragile"]
    print(f"{int(ff.sum())} of {len(P)} points fragile")
    assert ff.sum() <= 0.01 * len(P)
    assert_bitwise(f.data.T[~ff], ref["fpfh"][~ff], "surface cloud FPFH")
