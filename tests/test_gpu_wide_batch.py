"""Batches of more than 64 frames: frame masks of two 64-bit words (csrc/tsdf.h FMASK_WORDS), up to 128 frames per
batch for a whole volume whose batches run directly.  Frame f is bit f & 63 of word f >> 6; a unit enters the batch's
work list once whichever word is touched first; the integrate loads a slice once, runs word 0's frames, then word 1's,
and stores once.

Every case is compared bit for bit -- unit keys, tsdf, weight, float64 colour (precision 32: colour against the oracle at
its existing 1e-4 tolerance) and both counters -- with the CPU oracle and with the same frames through set_batch(64).
The frames are small (160 x 120, and 156 x 120 for the chunked staging: a width that is no multiple of the 8-pixel tile),
2-cm voxels, a wall seen from an arc of ring poses."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bitwise

INTR = (160, 120, 140.0, 140.0, 79.5, 59.5)
RAGGED = (156, 120, 140.0, 140.0, 77.5, 59.5)
VOXEL, TRUNC = 0.02, 0.04
WORD, CAP = 64, 128               # csrc/tsdf.h WORD_FRAMES, MAX_BATCH
COUNTS = (1, 63, 64, 65, 66, 127, 128, 129, 130)
HOOKS = ("otx_slice_pretest", "otx_integrate_workgroup", "otx_integrate_fine", "otx_integrate_depth")
TOUCH_FRAMES = 2                  # csrc/tsdf_touch.h TF: otx_touch_frames has no "default" value to go back to
_cache = {}


# ------------------------------------------------------------------------------------------------------- frames
def _scene(synth):
    return synth.Scene(boxes=[synth.Box((-0.2, -3.0, 0.0), (0.0, 3.0, 3.0))], ring_radius=1.0, cam_height=0.9,
                       look_height=0.9, seed=5)


def arc(synth, intr, poses):
    """(depth u16, colour, extrinsic) per ring pose of `poses` (of 64 around the wall), rendered once"""
    key = ("arc", intr, tuple(poses))
    if key not in _cache:
        scene, out = _scene(synth), []
        for i, k in enumerate(poses):
            T = synth.camera_pose(scene, k, 64)
            d, c = synth.render(scene, T, intr, frame_id=i)
            out.append((d, c, np.linalg.inv(T)))
        _cache[key] = out
    return _cache[key]


def sweep(n):
    """an arc swept back and forth: every frame sees most of the units its neighbours see"""
    return tuple(i % 17 - 8 for i in range(n))


def two_views(n=CAP):
    """the first 64 frames look at one end of the wall, the rest at the other; the middle is seen by both"""
    return tuple(i % 9 - 14 if i < WORD else i % 9 + 6 for i in range(n))


# ------------------------------------------------------------------------------------------------------- both sides
def oracle(O, name, intr, frames, counts=None):
    """the oracle's volume after the first n frames for each n of `counts` (default: all of them), from one pass;
    computed once per name and read-only"""
    counts = tuple(counts or (len(frames),))
    if ("ref", name) not in _cache:
        ref, out = O.TSDF(VOXEL, TRUNC, 1, 4), {}
        for i, (d, c, e) in enumerate(frames[:max(counts)]):
            ref.integrate(O.depth_to_float(d, 1000.0, 3.0), c, intr, e)
            if i + 1 in counts:
                snap = ref.export() + (ref.total_updates(), ref.unit_integrations())
                for a in snap[:4]:
                    a.setflags(write=False)
                out[i + 1] = snap
        _cache[("ref", name)] = out
    return _cache[("ref", name)]


def volume(pkg, batch, precision=64, **kw):
    integ = pkg.pipelines.integration
    return integ.ScalableTSDFVolume(voxel_length=VOXEL, sdf_trunc=TRUNC, color_type=integ.TSDFVolumeColorType.RGB8,
                                    batch_frames=batch, color_precision=precision, **kw)


def integrate(pkg, vol, intr, frames):
    pin = pkg.camera.PinholeCameraIntrinsic(*intr)
    G = pkg.geometry
    for d, c, e in frames:
        vol.integrate(G.RGBDImage.create_from_color_and_depth(G.Image(c), G.Image(d), depth_scale=1000.0,
                                                              depth_trunc=3.0, convert_rgb_to_intensity=False), pin, e)


def state(vol):
    """the volume's units and counters (flushes the queued frames)"""
    return [t.cpu().numpy() for t in vol.export_units(color_dtype="float64")] + list(vol.counters())


def compare(got, ref, precision=64, what=""):
    """a volume's state against the oracle's"""
    assert_bitwise(got[0], ref[0], what + "unit keys")
    assert len({tuple(k) for k in got[0].tolist()}) == got[0].shape[0], what + "a unit appears twice"
    assert_bitwise(got[2], ref[2], what + "voxel weights")
    assert_bitwise(got[1], ref[1], what + "voxel tsdf")
    if precision == 64:
        assert_bitwise(got[3], ref[3], what + "voxel colours (float64)")
    else:
        np.testing.assert_allclose(got[3], ref[3], rtol=1e-4, atol=1e-4 * 255)
    assert got[4] == ref[4], what + "voxel updates"
    assert got[5] == ref[5], what + "unit integrations"


def same(a, b, what=""):
    """two volumes' states, bit for bit at either colour precision"""
    for x, y, name in zip(a[:4], b[:4], ("unit keys", "voxel tsdf", "voxel weights", "voxel colours")):
        assert_bitwise(x, y, what + name)
    assert a[4:] == b[4:], what + "counters"


def batches(pkg, vol):
    n, units, new = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    pkg._lib.call("ot_tsdf_batch_stats", vol._h, C.byref(n), C.byref(units), C.byref(new))
    return n.value


def dropped(pkg, vol):
    out = (C.c_uint64 * 4)()
    pkg._lib.call("otx_tsdf_stats", vol._h, out)
    return int(out[2])


@pytest.fixture
def hooks(pkg):
    """set test hooks for one test; all back to their defaults afterwards"""
    L = pkg._lib

    def set_(**values):
        for hook, value in values.items():
            L.call(hook, value)

    yield set_
    for hook in HOOKS:
        L.call(hook, -1)
    L.call("otx_touch_frames", TOUCH_FRAMES)


def run(pkg, intr, frames, batch, precision=64, **kw):
    vol = volume(pkg, batch, precision, **kw)
    integrate(pkg, vol, intr, frames)
    return vol, state(vol)


# ------------------------------------------------------------------------------------------------------- cases
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", COUNTS)
def test_frame_counts(pkg, O, gpu, synth, n, precision):
    """1 to 130 frames at cap 128: one word, the word boundary, one and two frames into word 1, a full batch, and a
    second batch behind it.  The batch count says the wide batch ran: ceil(n / 128)."""
    frames = arc(synth, INTR, sweep(130))
    ref = oracle(O, "sweep", INTR, frames, COUNTS)[n]
    vol, wide = run(pkg, INTR, frames[:n], CAP, precision)
    assert batches(pkg, vol) == (n + CAP - 1) // CAP
    compare(wide, ref, precision)
    vol64, narrow = run(pkg, INTR, frames[:n], WORD, precision)
    assert batches(pkg, vol64) == (n + WORD - 1) // WORD
    same(wide, narrow)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("cap,intr,name", [(65, INTR, "sweep"), (96, RAGGED, "ragged"), (127, INTR, "sweep"),
                                           (128, RAGGED, "ragged")])
def test_caps(pkg, O, gpu, synth, cap, intr, name, precision):
    """130 frames at caps 65, 96 and 127 (batches that end one frame, half way and one frame short of word 1's end),
    and the ragged width, whose frames are staged by pixel chunks with the tile-max map from a second read."""
    frames = arc(synth, intr, sweep(130))
    ref = oracle(O, name, intr, frames, COUNTS if name == "sweep" else None)[130]
    vol, got = run(pkg, intr, frames, cap, precision)
    assert batches(pkg, vol) == (130 + cap - 1) // cap
    compare(got, ref, precision)
    same(got, run(pkg, intr, frames, WORD, precision)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("tf", [1, 3, 5, 7, 64])
def test_touch_groups_stay_in_one_word(pkg, O, gpu, synth, hooks, tf):
    """Frames per touch workgroup that do not divide 64 (otx_touch_frames): over a batch of more than 64 frames the group
    size falls to a divisor of 64, so no group's 64-bit mask straddles the words -- a frame on the wrong side would show
    as a unit with the wrong frames applied.  Both views, so units of either word and of both are there."""
    frames = arc(synth, INTR, two_views())
    hooks(otx_touch_frames=tf)
    vol, got = run(pkg, INTR, frames, CAP)
    assert batches(pkg, vol) == 1
    compare(got, oracle(O, "views", INTR, frames)[CAP])


def test_two_views_scene_has_units_of_each_kind(O, synth):
    """On the oracle alone: units seen only by frames 0..63, only by frames 64..127, and by both."""
    frames = arc(synth, INTR, two_views())
    first = {tuple(k) for k in oracle(O, "views0", INTR, frames[:WORD])[WORD][0].tolist()}
    second = {tuple(k) for k in oracle(O, "views1", INTR, frames[WORD:])[WORD][0].tolist()}
    assert first - second and second - first and first & second


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_units_of_either_word(pkg, O, gpu, synth, precision):
    """One 128-frame batch whose second half looks elsewhere: a unit touched through word 0 only, through word 1 only or
    through both is listed once (compare: no key twice, the oracle's unit integrations)."""
    frames = arc(synth, INTR, two_views())
    vol, got = run(pkg, INTR, frames, CAP, precision)
    assert batches(pkg, vol) == 1
    compare(got, oracle(O, "views", INTR, frames)[CAP], precision)
    same(got, run(pkg, INTR, frames, WORD, precision)[1])


@pytest.mark.gpu
def test_pretest_drops_the_same_wave_frames(pkg, O, gpu, synth, hooks):
    """The slice pre-test forced on.  It decides a (unit, slice, frame) triple from the frame's map alone, so a 128-frame
    batch drops what the same frames' two 64-frame batches drop: the same count, the same state and update count (the
    triples themselves are not read out: a different set of the same size would have to change no voxel either).  The
    volume held another scene before the reset, so a fresh unit whose frames are all dropped shows stale voxels unless
    it writes its zeros; the oracle says such units exist (touched, never updated)."""
    frames = arc(synth, INTR, two_views())
    ref = oracle(O, "views", INTR, frames)[CAP]
    assert (ref[2].max(axis=1) == 0).any()
    hooks(otx_slice_pretest=1, otx_integrate_fine=0)
    vol = volume(pkg, CAP)
    integrate(pkg, vol, INTR, arc(synth, INTR, sweep(130))[:CAP])
    vol.reset()
    integrate(pkg, vol, INTR, frames)
    wide = state(vol)
    assert batches(pkg, vol) == 1
    compare(wide, ref)
    vol64, narrow = run(pkg, INTR, frames, WORD)
    same(wide, narrow)
    assert dropped(pkg, vol) == dropped(pkg, vol64) > 0
    hooks(otx_slice_pretest=0)
    off, got = run(pkg, INTR, frames, CAP)
    same(wide, got)
    assert dropped(pkg, off) == 0


FORMS = {
    "fine1": {"otx_integrate_fine": 1, "otx_integrate_depth": 1},
    "fine2": {"otx_integrate_fine": 1, "otx_integrate_depth": 2},
    "fine3": {"otx_integrate_fine": 1, "otx_integrate_depth": 3},
    "wg1": {"otx_integrate_fine": 0, "otx_integrate_workgroup": 1, "otx_slice_pretest": 1},
    "wg2": {"otx_integrate_fine": 0, "otx_integrate_workgroup": 2, "otx_slice_pretest": 1},
    "wg4": {"otx_integrate_fine": 0, "otx_integrate_workgroup": 4, "otx_slice_pretest": 1},
}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("form", list(FORMS))
def test_forms(pkg, O, gpu, synth, hooks, form, precision):
    """The fine slices at each pipeline depth (the pipeline drains at the word boundary) and each workgroup form of the
    coarse integrate, over one 128-frame batch, then two frames more on the units' state."""
    frames = arc(synth, INTR, sweep(130))
    hooks(**FORMS[form])
    vol, got = run(pkg, INTR, frames, CAP, precision)
    assert batches(pkg, vol) == 2
    compare(got, oracle(O, "sweep", INTR, frames, COUNTS)[130], precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_pool_growth_inside_a_wide_batch(pkg, O, gpu, synth, precision):
    """A 64-unit pool: the 128-frame batch overflows it, the pool and the hash grow and the replay integrates the dropped
    units from the staged set (touch again through both words); then the grown volume again after a reset."""
    frames = arc(synth, INTR, two_views())
    ref = oracle(O, "views", INTR, frames)[CAP]
    assert ref[0].shape[0] > 64
    vol = volume(pkg, CAP, precision, max_units=64)
    integrate(pkg, vol, INTR, frames)
    compare(state(vol), ref, precision, what="grown: ")
    vol.reset()
    integrate(pkg, vol, INTR, frames)
    compare(state(vol), ref, precision, what="after reset: ")


@pytest.mark.gpu
def test_set_batch_between_batches(pkg, O, gpu, synth):
    """Batches of 128, then 4 and 4, then 128 frames of one volume."""
    frames = arc(synth, INTR, sweep(2 * CAP + 8))
    ref = oracle(O, "sweep264", INTR, frames)[len(frames)]
    vol = volume(pkg, CAP)
    at = 0
    for cap, n in ((CAP, CAP), (4, 8), (CAP, CAP)):
        vol.set_batch(cap)
        integrate(pkg, vol, INTR, frames[at:at + n])
        vol.flush()
        at += n
    assert batches(pkg, vol) == 4
    compare(state(vol), ref)


@pytest.mark.gpu
def test_sharded_volume_keeps_64(pkg, O, gpu, synth):
    """A sharded volume with set_batch(128) still batches by 64 (130 frames: three batches); each rank equals its
    set_batch(64) result and the ranks' union is the oracle's volume."""
    frames = arc(synth, INTR, sweep(130))
    ref = oracle(O, "sweep", INTR, frames, COUNTS)[130]
    parts = []
    for rank in range(2):
        got = []
        for cap in (CAP, WORD):
            vol = volume(pkg, cap)
            vol.set_shard(rank, 2)
            integrate(pkg, vol, INTR, frames)
            got.append(state(vol))
            assert batches(pkg, vol) == 3
        same(got[0], got[1], f"rank {rank}: ")
        parts.append(got[0])
    assert min(p[0].shape[0] for p in parts) > 0
    keys = np.concatenate([p[0] for p in parts])
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    union = [np.concatenate([p[i] for p in parts])[order] for i in range(4)]
    compare(union + [sum(p[4] for p in parts), sum(p[5] for p in parts)], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_last_table_entry(pkg, O, gpu, synth, precision):
    """A static camera, 128 frames in one batch on a fresh volume: the voxels every frame sees reach weight 128 = frames
    since reset + the batch, so the batch's last update reads the last entry of the reciprocal table it built."""
    frames = arc(synth, INTR, (0,)) * CAP
    ref = oracle(O, "static128", INTR, frames)[CAP]
    assert ref[2].max() == CAP
    vol, got = run(pkg, INTR, frames, CAP, precision)
    assert batches(pkg, vol) == 1
    compare(got, ref, precision)


@pytest.mark.gpu
def test_scan_call_starts_its_batch(pkg, O, gpu, synth):
    """ot_tsdf_integrate_u16_frames under the default cap: a scan of 64 frames (an object's) leaves nothing queued -- its
    batch starts before the call returns, not with the next reader -- 100 frames run as one batch, and 32 frames stay
    queued for the calls that follow, as frame-by-frame calls would leave them."""
    import torch

    L = pkg._lib
    frames = arc(synth, INTR, sweep(130))
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda().view(torch.uint16).contiguous()
    color = torch.from_numpy(np.stack([f[1] for f in frames])).cuda().contiguous()
    ext = np.ascontiguousarray(np.stack([f[2] for f in frames]), dtype=np.float64)
    intr = L.intrinsics_struct(pkg.camera.PinholeCameraIntrinsic(*INTR))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scan(vol, lo, hi):
        L.call("ot_tsdf_integrate_u16_frames", vol._h, hi - lo, depth.data_ptr() + lo * INTR[0] * INTR[1] * 2,
               color.data_ptr() + lo * INTR[0] * INTR[1] * 3, C.byref(intr), ext[lo:].ctypes.data, 1000.0, 3.0, stream)
        n = C.c_int32(-1)
        L.call("ot_tsdf_pending_frames", vol._h, C.byref(n))
        return n.value

    refs = oracle(O, "sweep", INTR, frames, COUNTS)
    vol = volume(pkg, None)
    assert scan(vol, 0, 64) == 0 and batches(pkg, vol) == 1
    compare(state(vol), refs[64])
    vol = volume(pkg, None)
    assert scan(vol, 0, 32) == 32 and scan(vol, 32, 63) == 63 and scan(vol, 63, 64) == 0
    assert batches(pkg, vol) == 1
    assert scan(vol, 64, 130) == 0 and batches(pkg, vol) == 2
    compare(state(vol), refs[130])
