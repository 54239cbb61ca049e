"""The coarse integrate's slice pre-test (csrc/slice_pretest.h, otx_slice_pretest): frames dropped from a slice's mask
before the frame loop, because the slice's bounding box in the image lies under depth that cannot make a candidate.
Every case is compared with the oracle bit for bit (unit keys, tsdf, weight, float64 colour; precision 32: colour at
its existing 1e-4 tolerance) and by both counters, with the hook at 1; where a case says so also with the hook at 0,
whose counters must be the same.  The count of dropped wave-frames (stats slot 2) must be above zero on the ring scans
and stay zero wherever the batch is not staged in full."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bitwise

TRUNC = 0.04
SMALL = ((160, 120, 141.400225, 141.400225, 80.125, 60.125), 0.01)   # a quarter of the reference camera, 10 mm
ODD = ((324, 243, 286.3, 286.3, 162.2, 121.7), 0.005)                # W % 8 != 0, H % 8 != 0: ragged tiles, 5 mm
_cache = {}


# ------------------------------------------------------------------------------------------------------- frames
def ring(synth, intr, n, ks=None):
    """frames ks of an n-frame ring around the box on the floor: depth u16, colour, extrinsics"""
    key = ("ring", intr, n, tuple(ks) if ks is not None else None)
    if key not in _cache:
        _cache[key] = synth.make_sequence(synth.Scene(), n_frames=n, intr=intr, frames=ks)
    return _cache[key]


def as_frames(depth, color, ext, float_depth=False):
    out = []
    for k in range(depth.shape[0]):
        d = depth[k]
        if float_depth and d.dtype != np.float32:
            d = (d.astype(np.float32) / np.float32(1000.0))
        out.append((d, color[k], ext[k]))
    return out


def oracle(O, name, cfg, frames, colored=True):
    """the oracle's volume after `frames`, computed once per name and read-only"""
    if ("ref", name) not in _cache:
        intr, voxel = cfg
        ref = O.TSDF(voxel, TRUNC, 1 if colored else 0, 4)
        for d, c, e in frames:
            f = d if d.dtype == np.float32 else O.depth_to_float(d, 1000.0, 3.0)
            ref.integrate(f, c if colored else None, intr, e)
        out = ref.export() + (ref.total_updates(), ref.unit_integrations())
        for a in out[:4]:
            a.setflags(write=False)
        _cache[("ref", name)] = out
    return _cache[("ref", name)]


def volume(pkg, cfg, batch=None, precision=64, colored=True, **kw):
    integ = pkg.pipelines.integration
    ct = integ.TSDFVolumeColorType.RGB8 if colored else integ.TSDFVolumeColorType.NoColor
    return integ.ScalableTSDFVolume(voxel_length=cfg[1], sdf_trunc=TRUNC, color_type=ct, batch_frames=batch,
                                    color_precision=precision, **kw)


def integrate(pkg, vol, cfg, frames):
    intr = pkg.camera.PinholeCameraIntrinsic(*cfg[0])
    G = pkg.geometry
    for d, c, e in frames:
        if d.dtype == np.float32:  # the float-depth entry (ot_tsdf_integrate)
            image = G.RGBDImage(G.Image(c), G.Image(d))
        else:
            image = G.RGBDImage.create_from_color_and_depth(G.Image(c), G.Image(d), depth_scale=1000.0,
                                                            depth_trunc=3.0, convert_rgb_to_intensity=False)
        vol.integrate(image, intr, e)


def dropped(pkg, vol):
    out = (C.c_uint64 * 4)()
    pkg._lib.call("otx_tsdf_stats", vol._h, out)
    return int(out[2])


def compare_arrays(got, ref, precision, colored=True):
    keys, tsdf, weight, col = got
    assert_bitwise(keys, ref[0], "unit keys")
    assert_bitwise(weight, ref[2], "voxel weights")
    assert_bitwise(tsdf, ref[1], "voxel tsdf")
    if not colored:
        assert not col.any()
    elif precision == 64:
        assert_bitwise(col, ref[3], "voxel colours (float64)")
    else:
        np.testing.assert_allclose(col, ref[3], rtol=1e-4, atol=1e-4 * 255)


def compare(vol, ref, colored=True):
    compare_arrays([t.cpu().numpy() for t in vol.export_units(color_dtype="float64")], ref, vol.color_precision,
                   colored)
    upd, units = vol.counters()
    assert upd == ref[4], "voxel updates"
    assert units == ref[5], "unit integrations"


HOOKS = ("otx_slice_pretest", "otx_integrate_workgroup", "otx_integrate_fine", "otx_split_frontend",
         "otx_defer_integrate")


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


def both_ways(pkg, hooks, cfg, frames, ref, expect_drops=True, **vol_args):
    """hook 1 against the oracle; hook 0 against the oracle too, with nothing dropped"""
    colored = vol_args.get("colored", True)
    hooks(otx_slice_pretest=1, otx_integrate_fine=0)
    vol = volume(pkg, cfg, **vol_args)
    integrate(pkg, vol, cfg, frames)
    compare(vol, ref, colored)
    n = dropped(pkg, vol)
    if expect_drops:
        assert n > 0, "the pre-test dropped no wave-frame"
    hooks(otx_slice_pretest=0)
    off = volume(pkg, cfg, **vol_args)
    integrate(pkg, off, cfg, frames)
    compare(off, ref, colored)
    assert dropped(pkg, off) == 0
    assert off.counters() == vol.counters()
    return n


# ------------------------------------------------------------------------------------------------------- cases
@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", [("small", SMALL), ("odd", ODD)])
@pytest.mark.parametrize("precision,colored", [(64, True), (32, True), (64, False)])
def test_ring(pkg, O, gpu, synth, hooks, name, cfg, precision, colored):
    """An 8-frame ring of the box on the floor as one batch, both colour precisions and without colour."""
    frames = as_frames(*ring(synth, cfg[0], 8))
    ref = oracle(O, ("ring8", name, colored), cfg, frames, colored)
    both_ways(pkg, hooks, cfg, frames, ref, precision=precision, colored=colored)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 64])
def test_batch_sizes(pkg, O, gpu, synth, hooks, batch):
    """70 frames: batches of one frame, and a batch of 64 then one of 6 (the set's maps hold 64 frames, then 6)."""
    frames = as_frames(*ring(synth, SMALL[0], 70))
    ref = oracle(O, "ring70", SMALL, frames)
    both_ways(pkg, hooks, SMALL, frames, ref, batch=batch)


@pytest.mark.gpu
def test_float_depth_with_invalid_pixels(pkg, O, gpu, synth, hooks):
    """The float-depth entry with negative, NaN and +inf pixels (+inf off the stride samples: Open3D's touch would
    unproject it): they enter the tile-max map as 0, 0 and +inf."""
    depth, color, ext = ring(synth, SMALL[0], 8)
    rng = np.random.default_rng(3)
    frames = []
    for d, c, e in as_frames(depth, color, ext, float_depth=True):
        d = d.copy()
        m = rng.random(d.shape)
        d[m < 0.03] = -0.7
        d[(m >= 0.03) & (m < 0.06)] = np.nan
        inf = (m >= 0.06) & (m < 0.065)
        inf[::4, ::4] = False
        d[inf] = np.inf
        frames.append((d, c, e))
    ref = oracle(O, "float_invalid", SMALL, frames)
    both_ways(pkg, hooks, SMALL, frames, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_ieee_division_kernel(pkg, O, gpu, synth, hooks, precision):
    """After an import the weights are arbitrary state and the integrate is the IEEE-division kernel: volume A takes
    the first four frames, volume B imports A's units and takes the other four with the pre-test on."""
    frames = as_frames(*ring(synth, SMALL[0], 8))
    ref = oracle(O, ("ring8", "small", True), SMALL, frames)
    hooks(otx_slice_pretest=1, otx_integrate_fine=0)
    a = volume(pkg, SMALL, precision=precision)
    integrate(pkg, a, SMALL, frames[:4])
    b = volume(pkg, SMALL, precision=precision, batch=3)
    b.import_units(*a.export_units())
    integrate(pkg, b, SMALL, frames[4:])
    compare_arrays([t.cpu().numpy() for t in b.export_units(color_dtype="float64")], ref, precision)
    assert dropped(pkg, b) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("wg", [1, 2, 4])
def test_workgroup_forms(pkg, O, gpu, synth, hooks, wg):
    frames = as_frames(*ring(synth, SMALL[0], 8))
    ref = oracle(O, ("ring8", "small", True), SMALL, frames)
    hooks(otx_integrate_workgroup=wg)
    both_ways(pkg, hooks, SMALL, frames, ref)


@pytest.mark.gpu
def test_replay_after_pool_growth(pkg, O, gpu, synth, hooks):
    """A 64-unit pool: the batch overflows it, the pool grows and the dropped units are integrated by the replay, from
    the staged frames and the set's maps of the first pass -- on a fresh volume and again after a reset."""
    frames = as_frames(*ring(synth, SMALL[0], 8))
    ref = oracle(O, ("ring8", "small", True), SMALL, frames)
    hooks(otx_slice_pretest=1, otx_integrate_fine=0)
    vol = volume(pkg, SMALL, max_units=64)
    integrate(pkg, vol, SMALL, frames[:3])
    assert vol.num_units() > 64
    vol.reset()
    integrate(pkg, vol, SMALL, frames)
    compare(vol, ref)
    assert dropped(pkg, vol) > 0
    fresh = volume(pkg, SMALL, max_units=64)
    integrate(pkg, fresh, SMALL, frames)
    compare(fresh, ref)


@pytest.mark.gpu
def test_split_front_end_takes_the_old_path(pkg, O, gpu, synth, hooks):
    """A sector-sharded volume with the split front end stages only its units' tiles: no map, nothing dropped, and the
    union of the ranks' units is the oracle's volume.  The same for a whole volume with the split front end forced."""
    depth, color, ext = ring(synth, SMALL[0], 8)
    frames = as_frames(depth, color, ext)
    ref = oracle(O, ("ring8", "small", True), SMALL, frames)
    hooks(otx_slice_pretest=1, otx_split_frontend=1)
    parts = []
    for rank in range(2):
        vol = volume(pkg, SMALL, batch=4)
        vol.set_shard_sector(rank, 2, (0.0, 0.0))
        integrate(pkg, vol, SMALL, frames)
        parts.append([t.cpu().numpy() for t in vol.export_units(color_dtype="float64")])
        assert dropped(pkg, vol) == 0
    assert min(p[0].shape[0] for p in parts) > 0
    keys = np.concatenate([p[0] for p in parts])
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    compare_arrays([np.concatenate([p[i] for p in parts])[order] for i in range(4)], ref, 64)
    whole = volume(pkg, SMALL, batch=4)
    integrate(pkg, whole, SMALL, frames)
    compare(whole, ref)
    assert dropped(pkg, whole) == 0


@pytest.mark.gpu
def test_camera_inside_the_volume(pkg, O, gpu, hooks):
    """A camera inside the units it touches: a patch of depth 6 cm in front of it (its unit holds the camera, with
    slices behind the image plane and beside every border), the rest of the image a wall at 0.9 m; four frames from
    cameras a few centimetres apart."""
    intr = SMALL[0]
    w, h = intr[:2]
    rng = np.random.default_rng(11)
    frames = []
    for i in range(4):
        d = np.full((h, w), 900, np.uint16)
        d[40:80, 50:110] = 60
        d[rng.random((h, w)) < 0.02] = 0
        E = np.eye(4)
        E[:3, 3] = (0.013 * i, -0.021 * i, 0.05 + 0.017 * i)
        frames.append((d, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), E))
    ref = oracle(O, "inside", SMALL, frames)
    assert ref[0].shape[0] > 20
    both_ways(pkg, hooks, SMALL, frames, ref, expect_drops=False)
