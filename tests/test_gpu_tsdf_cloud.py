"""GPU parity of ScalableTSDFVolume.extract_point_cloud / extract_voxel_point_cloud (tsdf_cloud.hip) against the numpy
restatement tests/tsdf_cloud_ref.py, bit for bit: every operation is a correctly rounded
IEEE operation in a fixed order, so there is no tolerance.  Everything goes through the facade, and so the C ABI.

The fixture volumes are built with import_units into a fresh, unsharded volume -- which is also how
distributed.assemble_sharded_volume builds the volume it returns."""
import numpy as np
import pytest

import tsdf_cloud_ref as R
from conftest import assert_bitwise, ref_intr

pytestmark = pytest.mark.gpu


def _host(t):
    return t.cpu().numpy()


def _import(pkg, units, vl, trunc=0.04, rgb=True, precision=64):
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = units
    ct = integ.TSDFVolumeColorType.RGB8 if rgb else integ.TSDFVolumeColorType.NoColor
    vol = integ.ScalableTSDFVolume(voxel_length=vl, sdf_trunc=trunc, color_type=ct, color_precision=precision)
    vol.import_units(keys, tsdf, weight, color if rgb else None)
    return vol


def _check_surface(pcd, ref, what, normals_at=None):
    assert len(pcd) == len(ref["points"]), f"{what}: {len(pcd)} points, the restatement has {len(ref['points'])}"
    assert_bitwise(np.asarray(pcd.points), ref["points"], what + " points")
    assert pcd.has_normals()
    nrm = np.asarray(pcd.normals)
    assert_bitwise(nrm if normals_at is None else nrm[normals_at], ref["normals"], what + " normals")
    if ref["colors"] is None:
        assert not pcd.has_colors()
    else:
        assert_bitwise(np.asarray(pcd.colors), ref["colors"], what + " colours")


def _check_voxel(pcd, ref, what):
    vp, vc = ref
    assert len(pcd) == len(vp), f"{what}: {len(pcd)} points, the restatement has {len(vp)}"
    assert_bitwise(np.asarray(pcd.points), vp, what + " points")
    assert_bitwise(np.asarray(pcd.colors), vc, what + " colours")
    assert not pcd.has_normals()


@pytest.fixture(scope="module")
def sphere():
    units = R.sphere_units()
    keys, tsdf, weight, color = units
    return units, R.extract_point_cloud(keys, tsdf, weight, color, R.SPHERE_VL), \
        R.extract_voxel_point_cloud(keys, tsdf, weight, R.SPHERE_VL)


def test_sphere_fixture_bitexact(pkg, gpu, sphere):
    units, ref, vref = sphere
    vol = _import(pkg, units, R.SPHERE_VL)
    pcd = vol.extract_point_cloud()
    assert len(pcd) == 1800
    _check_surface(pcd, ref, "sphere")
    vox = vol.extract_voxel_point_cloud()
    assert len(vox) == 9840
    _check_voxel(vox, vref, "sphere voxels")


def test_sphere_fixture_colour_precision_32_and_nocolor(pkg, gpu, sphere):
    units, ref, vref = sphere
    keys, tsdf, weight, color = units
    v32 = _import(pkg, (keys, tsdf, weight, color.astype(np.float32)), R.SPHERE_VL, precision=32)
    assert v32.color_precision == 32
    _check_surface(v32.extract_point_cloud(), ref, "sphere, float32 colour state")
    _check_voxel(v32.extract_voxel_point_cloud(), vref, "sphere voxels, float32 colour state")
    vnc = _import(pkg, units, R.SPHERE_VL, rgb=False)
    pcd = vnc.extract_point_cloud()
    assert pcd.has_normals() and not pcd.has_colors()
    _check_surface(pcd, dict(ref, colors=None), "sphere, NoColor")
    _check_voxel(vnc.extract_voxel_point_cloud(), vref, "sphere voxels, NoColor")


def test_sphere_fixture_shifted_keys(pkg, gpu):
    """negative and positive keys, other hash slots"""
    units = R.sphere_units(shift=(3, -5, 2))
    keys, tsdf, weight, color = units
    assert keys.min() < 0 < keys.max()
    vol = _import(pkg, units, R.SPHERE_VL)
    ref = R.extract_point_cloud(keys, tsdf, weight, color, R.SPHERE_VL)
    assert len(ref["points"]) == 1800
    _check_surface(vol.extract_point_cloud(), ref, "shifted sphere")
    _check_voxel(vol.extract_voxel_point_cloud(), R.extract_voxel_point_cloud(keys, tsdf, weight, R.SPHERE_VL),
                 "shifted sphere voxels")


def test_slab_fixture_bitexact(pkg, gpu):
    """normals exactly (0, 0, +-1): the lateral differences are exact zeros on the GPU too"""
    units = R.slab_units()
    keys, tsdf, weight, _ = units
    vol = _import(pkg, units, R.SLAB_VL, trunc=4 * R.SLAB_VL, rgb=False)
    ref = R.extract_point_cloud(keys, tsdf, weight, None, R.SLAB_VL)
    pcd = vol.extract_point_cloud()
    _check_surface(pcd, ref, "slab")
    assert np.all(np.abs(np.asarray(pcd.normals)) == np.array([0.0, 0.0, 1.0]))


def test_dense_units_bitexact(pkg, gpu):
    """more points in a unit than the emission lists in LDS at a time (2048): the chunked path, across a unit border"""
    units = R.dense_units()
    keys, tsdf, weight, color = units
    ref = R.extract_point_cloud(keys, tsdf, weight, color, 0.01)
    per_unit = np.bincount(ref["edge"][:, 0], minlength=2)
    assert per_unit.min() > 2 * 2048 + 256  # three chunks or more in both units, the last one partial
    vol = _import(pkg, units, 0.01)
    _check_surface(vol.extract_point_cloud(), ref, "dense units")
    _check_voxel(vol.extract_voxel_point_cloud(), R.extract_voxel_point_cloud(keys, tsdf, weight, 0.01),
                 "dense units voxels")


def _frames(pkg, synth, seq16):
    depth, color, ext = seq16
    intr = pkg.camera.PinholeCameraIntrinsic(*ref_intr(synth))
    rgbd = [pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(color[k]), pkg.geometry.Image(depth[k]), depth_scale=1000.0, depth_trunc=3.0,
        convert_rgb_to_intensity=False) for k in range(depth.shape[0])]
    return rgbd, intr, ext


@pytest.mark.parametrize("voxel", [0.01, 0.005])
def test_scan_bitexact(pkg, synth, seq16, gpu, voxel):
    """four 640x480 frames, default batching, no explicit flush before the extraction"""
    integ = pkg.pipelines.integration
    rgbd, intr, ext = _frames(pkg, synth, seq16)
    vol = integ.ScalableTSDFVolume(voxel_length=voxel, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)
    for k in range(len(rgbd)):
        vol.integrate(rgbd[k], intr, ext[k])
    pcd = vol.extract_point_cloud()
    vox = vol.extract_voxel_point_cloud()
    # (float)color_ is the float64 state narrowed to float32: exactly what the float32 export rounds to
    keys, tsdf, weight, color = (_host(a) for a in vol.export_units(color_dtype="float32"))
    assert len(pcd) > 1000
    sel = np.arange(0, len(pcd), 37)
    ref = R.extract_point_cloud(keys, tsdf, weight, color, voxel, normals_at=sel)
    _check_surface(pcd, ref, f"scan {voxel}", normals_at=sel)
    _check_voxel(vox, R.extract_voxel_point_cloud(keys, tsdf, weight, voxel), f"scan {voxel} voxels")


def test_readers_do_not_disturb_one_another(pkg, synth, seq16, gpu):
    import ctypes as C

    integ = pkg.pipelines.integration
    L = pkg._lib
    rgbd, intr, ext = _frames(pkg, synth, seq16)
    vol = integ.ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)
    for k in range(3):
        vol.integrate(rgbd[k], intr, ext[k])
    mesh = vol.extract_triangle_mesh()
    serial = C.c_int64(-2)
    L.call("ot_tsdf_mesh_serial", vol._h, C.byref(serial))
    cloud = vol.extract_point_cloud()
    vox = vol.extract_voxel_point_cloud()
    after = C.c_int64(-2)
    L.call("ot_tsdf_mesh_serial", vol._h, C.byref(after))
    assert after.value == serial.value >= 0  # the marching-cubes structure is still the mesh's
    mesh.compute_vertex_normals()
    fresh = vol.extract_triangle_mesh()
    fresh.compute_vertex_normals()
    assert_bitwise(np.asarray(mesh.vertices), np.asarray(fresh.vertices), "vertices")
    assert_bitwise(np.asarray(mesh.triangles), np.asarray(fresh.triangles), "triangles")
    assert_bitwise(np.asarray(mesh.vertex_normals), np.asarray(fresh.vertex_normals), "vertex normals")
    again = vol.extract_point_cloud()
    assert_bitwise(np.asarray(again.points), np.asarray(cloud.points), "second extraction, points")
    assert_bitwise(np.asarray(again.normals), np.asarray(cloud.normals), "second extraction, normals")
    assert_bitwise(np.asarray(again.colors), np.asarray(cloud.colors), "second extraction, colours")
    vox2 = vol.extract_voxel_point_cloud()
    assert_bitwise(np.asarray(vox2.points), np.asarray(vox.points), "second extraction, voxel points")
    # an emission after the volume changed is refused at the C level ...
    vol.integrate(rgbd[3], intr, ext[3])
    vol.flush()
    torch = pkg._device.torch
    buf = torch.empty((len(cloud), 3), dtype=torch.float64, device="cuda")
    st = L.load().ot_tsdf_emit_point_cloud(vol._h, buf.data_ptr(), buf.data_ptr(), None, None)
    assert st == L.OT_ERR_INVALID_ARGUMENT and b"ExtractPointCloud" in L.load().ot_last_error()
    # ... and a new extraction sees the frame
    more = vol.extract_point_cloud()
    assert len(more) != len(cloud) or not np.array_equal(np.asarray(more.points), np.asarray(cloud.points))


def test_queued_frame_is_flushed(pkg, synth, seq16, gpu):
    integ = pkg.pipelines.integration
    rgbd, intr, ext = _frames(pkg, synth, seq16)
    vol = integ.ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)
    vol.integrate(rgbd[0], intr, ext[0])
    one = vol.extract_point_cloud()
    vone = vol.extract_voxel_point_cloud()
    vol.integrate(rgbd[1], intr, ext[1])  # queued: no flush
    two = vol.extract_point_cloud()
    assert len(one) > 0
    assert len(two) != len(one) or not np.array_equal(np.asarray(two.points), np.asarray(one.points))
    vol.integrate(rgbd[2], intr, ext[2])
    vtwo = vol.extract_voxel_point_cloud()
    assert len(vtwo) > len(vone) > 0


def test_empty_and_refused(pkg, synth, seq16, gpu):
    integ = pkg.pipelines.integration
    rgbd, intr, ext = _frames(pkg, synth, seq16)

    def make():
        return integ.ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)

    vol = make()
    for pcd in (vol.extract_point_cloud(), vol.extract_voxel_point_cloud()):
        assert len(pcd) == 0 and pcd.is_empty() and not pcd.has_normals() and not pcd.has_colors()
    vol.integrate(rgbd[0], intr, ext[0])
    assert len(vol.extract_point_cloud()) > 0
    vol.reset()
    for pcd in (vol.extract_point_cloud(), vol.extract_voxel_point_cloud()):
        assert len(pcd) == 0 and pcd.is_empty()
    shard = make()
    shard.set_shard_sector(0, 2)
    shard.integrate(rgbd[0], intr, ext[0])
    with pytest.raises(RuntimeError, match="assemble_sharded_volume"):
        shard.extract_point_cloud()
    with pytest.raises(RuntimeError, match="assemble_sharded_volume"):
        shard.extract_voxel_point_cloud()
