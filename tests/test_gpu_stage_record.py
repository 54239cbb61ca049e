"""The 8-byte staged record (depth, colour) with the ray multiplier gathered from the volume's one table by the lanes
that can update, and the reciprocal table filled only up to the batch's largest weight + 1: a wide camera (corner
multiplier 1.6, so the candidate test on d - z and Open3D's test on (d - z) * m differ for many voxels), the slow
staging paths, the forced front-end / slice forms and the table bound -- all bitwise against the oracle through the
C ABI (keys, tsdf, weight, float64 colour, both counters)."""
import numpy as np
import pytest

from conftest import assert_bitwise

pytestmark = pytest.mark.gpu

WIDE = (64, 48, 32.0, 32.0, 31.5, 23.5)  # 90 x 74 degrees: multiplier up to sqrt(1 + 0.75^2 + 1) = 1.6
ODD = (63, 47, 32.0, 32.0, 31.0, 23.0)   # pixel count not a multiple of 4: the per-pixel staging paths
VOXEL, TRUNC = 0.01, 0.04
_cache = {}


def _wall_scene(synth):
    # a 6 m x 3 m wall in the plane x = 0, seen from x > 0: it fills every frame below
    return synth.Scene(boxes=[synth.Box((-0.2, -3.0, 0.0), (0.0, 3.0, 3.0))], ring_radius=1.0, cam_height=0.9,
                       look_height=0.9, seed=11)


def _frames(synth, intr_t, ks, n_ring=64):
    """frames at ring positions ks of n_ring (a short orbit around the wall's normal): depth u16, colour, extrinsics"""
    key = ("frames", intr_t, tuple(ks))
    if key not in _cache:
        scene = _wall_scene(synth)
        dep, col, ext = [], [], []
        for i, k in enumerate(ks):
            T = synth.camera_pose(scene, k, n_ring)
            d, c = synth.render(scene, T, intr_t, frame_id=i)
            dep.append(d), col.append(c), ext.append(np.linalg.inv(T))
        _cache[key] = (np.stack(dep), np.stack(col), np.stack(ext))
    return _cache[key]


ORBIT = (-3, -2, -1, 0, 1, 2)  # 6 poses, +-17 degrees


def _oracle(O, synth, intr_t, ks, colored, trunc=3.0):
    """the oracle's volume for a frame list, computed once and shared (read-only)"""
    key = ("ref", intr_t, tuple(ks), colored)
    if key not in _cache:
        depth, color, ext = _frames(synth, intr_t, ks)
        ref = O.TSDF(VOXEL, TRUNC, 1 if colored else 0, 4)
        for k in range(depth.shape[0]):
            ref.integrate(O.depth_to_float(depth[k], 1000.0, trunc), color[k] if colored else None, intr_t, ext[k])
        out = ref.export() + (ref.total_updates(), ref.unit_integrations())
        for a in out[:4]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _volume(pkg, colored, batch, precision=64):
    integ = pkg.pipelines.integration
    ct = integ.TSDFVolumeColorType.RGB8 if colored else integ.TSDFVolumeColorType.NoColor
    return integ.ScalableTSDFVolume(voxel_length=VOXEL, sdf_trunc=TRUNC, color_type=ct, batch_frames=batch,
                                    color_precision=precision)


def _integrate(pkg, vol, intr_t, depth, color, ext, float_path=False, trunc=3.0):
    intr = pkg.camera.PinholeCameraIntrinsic(*intr_t)
    for k in range(depth.shape[0]):
        rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
            pkg.geometry.Image(color[k]), pkg.geometry.Image(depth[k]), depth_scale=1000.0, depth_trunc=trunc,
            convert_rgb_to_intensity=False)
        if float_path:
            rgbd._raw_depth = None  # the float-depth entry point (ot_tsdf_integrate)
        vol.integrate(rgbd, intr, ext[k])


def _compare(vol, ref, colored):
    rk, rt, rw, rc, rupd, runits = ref
    keys, tsdf, weight, col = (t.cpu().numpy() for t in vol.export_units(color_dtype="float64"))
    assert_bitwise(keys, rk, "unit keys")
    assert_bitwise(weight, rw, "voxel weights")
    assert_bitwise(tsdf, rt, "voxel tsdf")
    if not colored:
        assert not col.any()
    elif vol.color_precision == 64:
        assert_bitwise(col, rc, "voxel colours (float64)")
    else:  # float32 state with one reciprocal per update (the existing tolerance of the precision-32 mode)
        np.testing.assert_allclose(col, rc, rtol=1e-4, atol=1e-4 * 255)
    upd, units = vol.counters()
    assert upd == rupd
    assert units == runits
    return keys.shape[0]


def _run(pkg, O, synth, intr_t, ks, colored=True, batch=None, precision=64, float_path=False):
    depth, color, ext = _frames(synth, intr_t, ks)
    vol = _volume(pkg, colored, batch, precision)
    _integrate(pkg, vol, intr_t, depth, color, ext, float_path)
    return _compare(vol, _oracle(O, synth, intr_t, ks, colored), colored)


@pytest.mark.parametrize("batch", [1, 4, None])
@pytest.mark.parametrize("colored,precision", [(True, 64), (True, 32), (False, 64)])
def test_wide_fov_scan(pkg, O, gpu, synth, batch, colored, precision):
    depth, _, _ = _frames(synth, WIDE, ORBIT)
    mult = O.depth_multiplier(*WIDE)
    wide = (depth[0] > 0) & (depth[0] < 3000) & (mult >= np.float32(1.25))
    assert int(wide.sum()) >= 1000, "the scan must put valid depth on pixels with a large multiplier"
    assert _run(pkg, O, synth, WIDE, ORBIT, colored, batch, precision) > 100


@pytest.mark.parametrize("batch,float_path", [(1, False), (4, False), (4, True)])
def test_slow_staging_paths(pkg, O, gpu, synth, batch, float_path):
    """63 x 47 pixels (not a multiple of 4: prep_quad's per-pixel fallback), and the float-depth entry point"""
    assert (ODD[0] * ODD[1]) % 4 != 0
    assert _run(pkg, O, synth, ODD, ORBIT, True, batch, 64, float_path) > 100


def test_float_depth_wide(pkg, O, gpu, synth):
    assert _run(pkg, O, synth, WIDE, ORBIT, True, 4, 64, float_path=True) > 100


@pytest.mark.parametrize("defer", [0, 1])
def test_split_frontend_forced(pkg, O, gpu, synth, defer):
    L = pkg._lib
    L.call("otx_split_frontend", 1)
    L.call("otx_defer_integrate", defer)
    try:
        assert _run(pkg, O, synth, WIDE, ORBIT, True, 4) > 100
    finally:
        L.call("otx_split_frontend", -1)
        L.call("otx_defer_integrate", -1)


def _integrate_pairs(pkg, synth, vol, before_batch):
    """the orbit in batches of 2 (the volume's batch_frames; the second frame of a pair flushes it without joining, so a
    deferred batch stays pending); before_batch(b) runs ahead of batch b's frames"""
    depth, color, ext = _frames(synth, WIDE, ORBIT)
    for b in range(len(ORBIT) // 2):
        before_batch(b)
        s = slice(2 * b, 2 * b + 2)
        _integrate(pkg, vol, WIDE, depth[s], color[s], ext[s])


@pytest.mark.parametrize("defers", [(1, 0, 1), (1, 1, 0), (0, 1, 1)])
def test_defer_mode_changes_between_batches(pkg, O, gpu, synth, defers):
    """Three batches of 2 with the split front end, otx_defer_integrate set per batch (between batches, nothing flushes):
    a pending deferred batch that the next batch does not fuse with is launched alone before that batch restages
    anything, so every sequence gives the oracle's volume.  (Before integrate_batch owned the hand-over, (1, 0, 1) left
    batch 0 pending behind the direct batch 1, which restaged its set: the third batch then integrated batch 1's frames
    a second time and batch 0 was lost.)"""
    L = pkg._lib
    L.call("otx_split_frontend", 1)
    try:
        vol = _volume(pkg, True, 2)
        _integrate_pairs(pkg, synth, vol, lambda b: L.call("otx_defer_integrate", defers[b]))
        assert _compare(vol, _oracle(O, synth, WIDE, ORBIT, True), True) > 100
    finally:
        L.call("otx_split_frontend", -1)
        L.call("otx_defer_integrate", -1)


def test_overlap_set_behind_a_deferred_batch(pkg, O, gpu, synth):
    """ot_tsdf_set_frontend_overlap(1) through the C API (the facade would flush first) while the first batch is still
    deferred: the next batch runs double-buffered and launches the deferred one alone first."""
    L = pkg._lib
    L.call("otx_split_frontend", 1)
    L.call("otx_defer_integrate", 1)
    try:
        vol = _volume(pkg, True, 2)

        def before_batch(b):
            if b == 1:
                L.call("ot_tsdf_set_frontend_overlap", vol._h, 1)

        _integrate_pairs(pkg, synth, vol, before_batch)
        assert _compare(vol, _oracle(O, synth, WIDE, ORBIT, True), True) > 100
    finally:
        L.call("otx_split_frontend", -1)
        L.call("otx_defer_integrate", -1)


@pytest.mark.parametrize("reset", ["sync", "async"])
def test_reset_behind_a_deferred_scan(pkg, O, gpu, synth, reset):
    """A deferred scan (its last batch still pending), then the synchronous reset (ot_tsdf_reset drops the pending batch
    with the old contents) or the stream-ordered one (it integrates it first), then the scan again: the oracle's volume
    and counters both times -- both resets return the host state to the same start."""
    import torch

    L = pkg._lib
    L.call("otx_split_frontend", 1)
    L.call("otx_defer_integrate", 1)
    try:
        vol = _volume(pkg, True, 2)
        _integrate_pairs(pkg, synth, vol, lambda b: None)
        if reset == "sync":
            torch.cuda.synchronize()
            L.call("ot_tsdf_reset", vol._h)
            vol._keep.clear()
        else:
            vol.reset()
        _integrate_pairs(pkg, synth, vol, lambda b: None)
        assert _compare(vol, _oracle(O, synth, WIDE, ORBIT, True), True) > 100
    finally:
        L.call("otx_split_frontend", -1)
        L.call("otx_defer_integrate", -1)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_fine_slices_forced(pkg, O, gpu, synth, depth):
    L = pkg._lib
    L.call("otx_integrate_fine", 1)
    L.call("otx_integrate_depth", depth)
    try:
        assert _run(pkg, O, synth, WIDE, ORBIT, True, 4) > 100
    finally:
        L.call("otx_integrate_fine", -1)
        L.call("otx_integrate_depth", -1)


FORMS = {  # hook -> value; the hooks not named stay at -1
    "coarse": {"otx_integrate_fine": 0},
    "fine1": {"otx_integrate_fine": 1, "otx_integrate_depth": 1},
    "fine2": {"otx_integrate_fine": 1, "otx_integrate_depth": 2},
    "fine3": {"otx_integrate_fine": 1, "otx_integrate_depth": 3},
    "deferred_coarse": {"otx_split_frontend": 1, "otx_defer_integrate": 1, "otx_integrate_fine": 0},
    "deferred_fine": {"otx_split_frontend": 1, "otx_defer_integrate": 1, "otx_integrate_fine": 1},
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("division", ["table", "ieee"])
@pytest.mark.parametrize("precision", [64, 32])
def test_every_integrate_instantiation(pkg, O, gpu, synth, precision, division, form):
    """Every instantiation of the integrate (colour precision x division form x slice form: k_batch_integrate coarse
    and fine at pipeline depths 1-3, k_integrate_touch and k_integrate_touch_fine) on the wide-camera wall scan.
    table: a fresh volume, 6 frames in batches of 4 -- a deferred batch is launched once fused with the next touch and
    once alone by the flush.  ieee: the route of test_ieee_division_kernel_after_import -- volume A integrates the
    first 3 frames and exports, volume B imports A's units (arbitrary state: the IEEE-division kernels) and integrates
    the other 3 in batches of 2 with the form forced; the oracle integrates all six (voxel state; B's counters are the
    oracle's for the last three frames)."""
    depth, color, ext = _frames(synth, WIDE, ORBIT)
    ref = _oracle(O, synth, WIDE, ORBIT, True)
    L = pkg._lib
    if division == "table":
        vol, first = _volume(pkg, True, 4, precision), 0
    else:
        a = _volume(pkg, True, None, precision)
        _integrate(pkg, a, WIDE, depth[:3], color[:3], ext[:3])
        vol, first = _volume(pkg, True, 2, precision), 3
        vol.import_units(*a.export_units())
        # the counters count a volume's own integrations, and both are sums over frames (voxel updates; (unit, frame)
        # integrations): A's are the oracle's for the first 3 frames, so B's must be the six-frame oracle's less those
        upd3, units3 = _oracle(O, synth, WIDE, ORBIT[:3], True)[4:]
        assert tuple(a.counters()) == (upd3, units3)
        ref = ref[:4] + (ref[4] - upd3, ref[5] - units3)
    try:
        for hook, value in FORMS[form].items():
            L.call(hook, value)
        _integrate(pkg, vol, WIDE, depth[first:], color[first:], ext[first:])
        assert _compare(vol, ref, True) > 100
    finally:
        for hook in ("otx_integrate_fine", "otx_integrate_depth", "otx_split_frontend", "otx_defer_integrate"):
            L.call(hook, -1)


def test_reciprocal_table_bound(pkg, O, gpu, synth):
    """9 frames from one pose in batches of 4 (4, 4, 1): voxels seen every time reach weight 9, the last entry the last
    batch's table holds (frames since reset + the batch's).  Then a reset and 3 more frames (the bound starts again
    from 0), against a fresh volume and the oracle."""
    nine, three = (0,) * 9, (0,) * 3
    depth, color, ext = _frames(synth, WIDE, nine)
    ref9 = _oracle(O, synth, WIDE, nine, True)
    assert ref9[2].max() == 9.0
    vol = _volume(pkg, True, 4)
    _integrate(pkg, vol, WIDE, depth, color, ext)
    assert _compare(vol, ref9, True) > 50
    vol.reset()
    d3, c3, e3 = _frames(synth, WIDE, three)
    _integrate(pkg, vol, WIDE, d3, c3, e3)
    ref3 = _oracle(O, synth, WIDE, three, True)
    assert ref3[2].max() == 3.0
    _compare(vol, ref3, True)
    fresh = _volume(pkg, True, 4)
    _integrate(pkg, fresh, WIDE, d3, c3, e3)
    a, b = vol.export_units(), fresh.export_units()
    for x, y, what in zip(a, b, ("keys", "tsdf", "weight", "colour")):
        assert_bitwise(x.cpu().numpy(), y.cpu().numpy(), what + " (after reset vs fresh volume)")
    assert vol.counters() == fresh.counters()
