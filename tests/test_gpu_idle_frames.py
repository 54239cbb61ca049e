"""Idle wave-frames: a wave of the coarse integrate leaves a frame as soon as none of its lanes is a candidate for any
of its voxels (no valid depth in front of the truncation band under the slice), before the multiplier gathers, the
reciprocal reads and the updates; the fine slices run the same per-voxel test and gather without leaving early.  The
scene makes such wave-frames on purpose -- a wall with a block of missing depth in some frames, units behind the wall
and units at the image border -- and every instantiation of the integrate is compared bitwise with the oracle through
the C ABI: unit keys, tsdf, weight, float64 colour and both counters."""
import numpy as np
import pytest

from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

INTR = (160, 120, 80.0, 80.0, 79.5, 59.5)  # 90 x 74 degrees
VOXEL, TRUNC = 0.005, 0.04                 # 8-cm units, one wave's slice 4 x 4 x 2 cm
POSES = (-3, -2, -1, 0, 1, 2, 3, 0)        # ring positions of 64: +-17 degrees around the wall's normal
HOLED = (2, 3, 5)                          # frames with the block of zero depth
HOLE = (slice(35, 85), slice(50, 120))     # rows, columns: 50 x 70 pixels, a slice at 1 m covers about 4 x 4
_cache = {}


def _frames(synth):
    if "frames" not in _cache:
        scene = synth.Scene(boxes=[synth.Box((-0.2, -3.0, 0.0), (0.0, 3.0, 3.0))], ring_radius=1.0, cam_height=0.9,
                            look_height=0.9, seed=11)
        dep, col, ext = [], [], []
        for i, k in enumerate(POSES):
            T = synth.camera_pose(scene, k, 64)
            d, c = synth.render(scene, T, INTR, frame_id=i)
            if i in HOLED:
                d[HOLE] = 0
            dep.append(d), col.append(c), ext.append(np.linalg.inv(T))
        _cache["frames"] = (np.stack(dep), np.stack(col), np.stack(ext))
    return _cache["frames"]


def _oracle(O, synth, lo, hi):
    """the oracle's volume after frames [lo, hi), computed once and shared (read-only)"""
    key = ("ref", lo, hi)
    if key not in _cache:
        depth, color, ext = _frames(synth)
        ref = O.TSDF(VOXEL, TRUNC, 1, 4)
        for k in range(lo, hi):
            ref.integrate(O.depth_to_float(depth[k], 1000.0, 3.0), color[k], INTR, ext[k])
        out = ref.export() + (ref.total_updates(), ref.unit_integrations())
        for a in out[:4]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def slice_weights(weight):
    """weight [U][4096] in export order (x * 256 + y * 16 + z) -> the largest weight of each of a unit's 16 coarse
    slices (one wave's voxels: an 8 x 8 patch of columns x 4 consecutive z), [U][2][2][4]"""
    w = np.asarray(weight).reshape(-1, 2, 8, 2, 8, 4, 4)
    return w.max(axis=(2, 4, 6))


def _volume(pkg, batch, precision=64):
    integ = pkg.pipelines.integration
    return integ.ScalableTSDFVolume(voxel_length=VOXEL, sdf_trunc=TRUNC, color_type=integ.TSDFVolumeColorType.RGB8,
                                    batch_frames=batch, color_precision=precision)


def _integrate(pkg, vol, depth, color, ext):
    intr = pkg.camera.PinholeCameraIntrinsic(*INTR)
    for k in range(depth.shape[0]):
        rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
            pkg.geometry.Image(color[k]), pkg.geometry.Image(depth[k]), depth_scale=1000.0, depth_trunc=3.0,
            convert_rgb_to_intensity=False)
        vol.integrate(rgbd, intr, ext[k])


def _compare(vol, ref):
    rk, rt, rw, rc, rupd, runits = ref
    keys, tsdf, weight, col = (t.cpu().numpy() for t in vol.export_units(color_dtype="float64"))
    assert_bitwise(keys, rk, "unit keys")
    assert_bitwise(weight, rw, "voxel weights")
    assert_bitwise(tsdf, rt, "voxel tsdf")
    if vol.color_precision == 64:
        assert_bitwise(col, rc, "voxel colours (float64)")
    else:  # float32 state with one reciprocal per update (the existing tolerance of the precision-32 mode)
        np.testing.assert_allclose(col, rc, rtol=1e-4, atol=1e-4 * 255)
    upd, units = vol.counters()
    assert upd == rupd
    assert units == runits


def test_scene_has_idle_wave_frames(O, synth):
    """On the oracle's volume alone: the scene exercises the skip.  (1) A unit with a slice nothing ever updated
    beside a slice that was updated: that wave was idle in every frame of the unit's mask.  (2) A slice whose largest
    weight is below its unit's: that wave was idle in some of the unit's frames only."""
    depth, _, _ = _frames(synth)
    assert all((depth[i][HOLE] == 0).all() for i in HOLED) and all((depth[i] > 0).mean() > 0.9 for i in range(len(POSES))
                                                                   if i not in HOLED)
    sw = slice_weights(_oracle(O, synth, 0, len(POSES))[2]).reshape(-1, 16)
    never = (sw == 0).any(axis=1) & (sw > 0).any(axis=1)
    partly = ((sw > 0) & (sw < sw.max(axis=1, keepdims=True))).any(axis=1)
    assert int(never.sum()) >= 50, "units with a never-updated slice beside an updated one"
    assert int(partly.sum()) >= 50, "units with a slice idle in some of the unit's frames only"


FORMS = {  # hook -> value; the hooks not named stay at -1
    "coarse": {"otx_integrate_fine": 0},
    "fine1": {"otx_integrate_fine": 1, "otx_integrate_depth": 1},
    "fine2": {"otx_integrate_fine": 1, "otx_integrate_depth": 2},
    "fine3": {"otx_integrate_fine": 1, "otx_integrate_depth": 3},
    "deferred_coarse": {"otx_split_frontend": 1, "otx_defer_integrate": 1, "otx_integrate_fine": 0},
    "deferred_fine": {"otx_split_frontend": 1, "otx_defer_integrate": 1, "otx_integrate_fine": 1},
}
HOOKS = ("otx_integrate_fine", "otx_integrate_depth", "otx_split_frontend", "otx_defer_integrate")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("division", ["table", "ieee"])
@pytest.mark.parametrize("precision", [64, 32])
def test_idle_frames_every_instantiation(pkg, O, gpu, synth, precision, division, form):
    """The scene through every instantiation of the integrate (colour precision x division form x slice form).
    table: a fresh volume, the 8 frames in batches of 3 (3, 3, 2: the second and third batch find the units' state in
    HBM, and a slice idle through a whole batch is not written back).  ieee: volume A integrates the first 3 frames
    and exports, volume B imports A's units (arbitrary state: the IEEE-division kernels) and integrates the other 5
    in batches of 3 with the form forced; B's counters are the oracle's for all frames less those of the first 3."""
    depth, color, ext = _frames(synth)
    n = len(POSES)
    ref = _oracle(O, synth, 0, n)
    L = pkg._lib
    if division == "table":
        vol, first = _volume(pkg, 3, precision), 0
    else:
        a = _volume(pkg, None, precision)
        _integrate(pkg, a, depth[:3], color[:3], ext[:3])
        vol, first = _volume(pkg, 3, precision), 3
        vol.import_units(*a.export_units())
        upd3, units3 = _oracle(O, synth, 0, 3)[4:]
        assert tuple(a.counters()) == (upd3, units3)
        ref = ref[:4] + (ref[4] - upd3, ref[5] - units3)
    try:
        for hook, value in FORMS[form].items():
            L.call(hook, value)
        _integrate(pkg, vol, depth[first:], color[first:], ext[first:])
        _compare(vol, ref)
    finally:
        for hook in HOOKS:
            L.call(hook, -1)


@pytest.mark.parametrize("batch", [1, None])
def test_idle_frames_batch_sizes(pkg, O, gpu, synth, batch):
    """one-frame batches (every idle slice of a known unit skips its write-back) and one batch for all 8 frames"""
    depth, color, ext = _frames(synth)
    vol = _volume(pkg, batch)
    _integrate(pkg, vol, depth, color, ext)
    _compare(vol, _oracle(O, synth, 0, len(POSES)))
