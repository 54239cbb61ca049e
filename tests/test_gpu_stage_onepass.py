"""The batch staging's one-pass form (csrc/tsdf_stage.h stage_tile_quads, otx_stage_onepass): an eligible frame (u16 depth,
16-B aligned, W % 8 == 0, colour absent or 4-B aligned) of a batch with tile-max maps is staged in 8 x 8 tile order and
its map words are reduced from the converted depths the lanes hold; every other frame keeps the two-pass form.
1. The staged records and map words, read back with otx_tsdf_staged, against a numpy model and between the two forms.
2. Whole volumes against the oracle, bit for bit, in both forms, with the same wave-frames dropped by the pre-test.
3. A pool that grows inside a batch: the replay reads the first pass's maps."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bitwise
from test_gpu_slice_pretest import SMALL, as_frames, compare, dropped, integrate, oracle, ring, volume

SCALE, TRUNC_M = 1000.0, 3.0
RAW = np.array([0, 1, 2999, 3000, 3001, 65535], np.uint16)  # around the truncation at 3.0 m, and the ends
TALL = ((168, 122, 148.5, 148.5, 84.1, 61.1), 0.01)         # W % 8 == 0, H % 8 == 2: ragged bottom tiles, one pass
HOOKS = ("otx_stage_onepass", "otx_touch_stage_blocks", "otx_slice_pretest", "otx_integrate_fine")


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
    L.call("otx_touch_frames", 2)


# ------------------------------------------------------------------------------------------------ 1. the read-out
def u16_frames(w, h, n, seed):
    """n frames of depths drawn from RAW and random colours.  Where the image has them: tile (0, 0) all zero, and
    tile (1, 0) -- the only tile of an 8 x 8 image -- with its largest raw value truncated away and a 1 surviving."""
    rng = np.random.default_rng(seed)
    depth = RAW[rng.integers(0, RAW.size, (n, h, w))]
    x0 = 8 if w >= 16 else 0
    depth[:, :8, x0:x0 + 8] = rng.integers(0, 2, (n, min(h, 8), 8)).astype(np.uint16)
    depth[:, 3, x0 + 5] = 3001
    depth[:, 6, x0 + 2] = 1
    if w >= 16:
        depth[:, :8, :8] = 0
    return depth, rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def float_frames(w, h, n, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.2, 2.9, (n, h, w)).astype(np.float32)
    m = rng.random((n, h, w))
    depth[m < 0.1] = 0.0
    depth[(m >= 0.1) & (m < 0.2)] = -1.0
    depth[(m >= 0.2) & (m < 0.3)] = np.nan
    inf = (m >= 0.3) & (m < 0.35)
    inf[:, ::4, ::4] = False  # (the touch would unproject a stride sample at +inf)
    depth[inf] = np.inf
    depth[:, :8, :8] = np.where(m[:, :8, :8] < 0.5, np.float32(-1.0), np.float32(np.nan))  # a tile with nothing > 0
    return depth, rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def model(depth, color):
    """the records (u64: float depth bits, colour word above them) and the map words of one frame"""
    if depth.dtype == np.uint16:
        d = depth.astype(np.float32) / np.float32(SCALE)
        d[d.astype(np.float64) >= TRUNC_M] = 0.0
    else:
        d = depth
    bits = np.ascontiguousarray(d).view(np.uint32)
    word = np.zeros(d.shape, np.uint64)
    if color is not None:
        c = color.astype(np.uint64)
        word = c[..., 0] | (c[..., 1] << np.uint64(8)) | (c[..., 2] << np.uint64(16))
    records = bits.astype(np.uint64) | (word << np.uint64(32))
    with np.errstate(invalid="ignore"):
        key = np.where(d > 0, bits, np.uint32(0))
    h, w = d.shape
    th, tw = -(-h // 8), -(-w // 8)
    pad = np.zeros((th * 8, tw * 8), np.uint32)
    pad[:h, :w] = key
    return records.ravel(), pad.reshape(th, 8, tw, 8).max(axis=(1, 3)).ravel()


def on_device(torch, arr, offset):
    """arr's bytes in device memory `offset` bytes past an aligned address: (the buffer, the address)"""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).ravel().copy())
    buf = torch.zeros(raw.numel() + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + raw.numel()] = raw.cuda()
    return buf, buf.data_ptr() + offset


def staged(pkg, w, h, depth, color, colored=True, d_off=None, c_off=None):
    """one batch of the frames through the C entry points; per frame the staged records and map words"""
    import torch

    L = pkg._lib
    n = depth.shape[0]
    d_off, c_off = d_off or [0] * n, c_off or [0] * n
    intr = L.ot_intrinsics(w, h, float(w), float(w), w / 2 - 0.5, h / 2 - 0.5)
    ext = np.eye(4)
    vol = C.c_void_p()
    # 0.64-m units: the random depths of a batch touch a few hundred at most
    L.call("ot_tsdf_create", 0.04, 0.16, L.OT_COLOR_RGB8 if colored else L.OT_COLOR_NONE, 16, 4, 0, C.byref(vol))
    keep = []
    try:
        for k in range(n):
            db, dp = on_device(torch, depth[k], d_off[k])
            keep.append(db)
            cp = None
            if colored:
                cb, cp = on_device(torch, color[k], c_off[k])
                keep.append(cb)
            if depth.dtype == np.uint16:
                L.call("ot_tsdf_integrate_u16", vol, dp, cp, C.byref(intr), ext.ctypes.data, SCALE, TRUNC_M, None)
            else:
                L.call("ot_tsdf_integrate", vol, dp, cp, C.byref(intr), ext.ctypes.data, None)
        out = []
        for k in range(n):
            rec = np.zeros(w * h, np.uint64)
            tmap = np.zeros((-(-w // 8)) * (-(-h // 8)), np.uint32)
            L.call("otx_tsdf_staged", vol, k, rec.ctypes.data, tmap.ctypes.data)
            out.append((rec, tmap))
        return out
    finally:
        L.call("ot_tsdf_destroy", vol)


#        name         W    H  frames  kind   colour  depth offsets  colour offsets
CASES = [("tile",       8,   8, 1, "u16",   True,  None,      None),
         ("group",     64,  48, 3, "u16",   True,  None,      None),       # a ragged two-frame group
         ("ragged",   328, 242, 2, "u16",   True,  None,      None),       # bottom tiles of two rows, one pass
         ("odd",      324, 243, 2, "u16",   True,  None,      None),       # W % 8 != 0: two passes
         ("nocolor",   64,  48, 2, "u16",   False, None,      None),
         ("float",     64,  48, 2, "float", True,  None,      None),       # two passes
         ("depth2",    64,  48, 2, "u16",   True,  [2, 2],    None),       # depth only 2-B aligned: two passes
         ("colour1",   64,  48, 2, "u16",   True,  None,      [1, 1]),     # colour only 1-B aligned: two passes
         ("mixed",     64,  48, 4, "u16",   True,  [0, 2, 0, 8], [0, 0, 3, 0])]  # both forms in one batch
_model = {}


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [-1, 0, 7])
@pytest.mark.parametrize("tf", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_staged_records_and_maps(pkg, gpu, hooks, case, tf, blocks):
    name, w, h, n, kind, colored, d_off, c_off = case
    if name not in _model:
        depth, color = (u16_frames if kind == "u16" else float_frames)(w, h, n, seed=CASES.index(case) + 1)
        _model[name] = (depth, color, [model(depth[k], color[k] if colored else None) for k in range(n)])
    depth, color, want = _model[name]
    hooks(otx_touch_stage_blocks=blocks, otx_touch_frames=tf, otx_slice_pretest=1)
    got = {}
    for onepass in (-1, 0):
        hooks(otx_stage_onepass=onepass)
        got[onepass] = staged(pkg, w, h, depth, color, colored, d_off, c_off)
        for k in range(n):
            assert_bitwise(got[onepass][k][0], want[k][0], f"{name} form {onepass} frame {k}: staged records")
            assert_bitwise(got[onepass][k][1], want[k][1], f"{name} form {onepass} frame {k}: map words")
    for k in range(n):
        assert_bitwise(got[-1][k][0], got[0][k][0], f"{name} frame {k}: records of the two forms")
        assert_bitwise(got[-1][k][1], got[0][k][1], f"{name} frame {k}: maps of the two forms")


@pytest.mark.gpu
def test_model_cases_hold_what_they_claim(pkg, gpu):
    """the inputs themselves: a tile whose largest raw depth is truncated while a smaller one survives, an all-zero
    tile, every value of RAW; and the read-out refuses a map the batch did not build"""
    depth, color = u16_frames(64, 48, 1, seed=5)
    assert set(np.unique(depth)) == set(RAW.tolist())
    records, tmap = model(depth[0], color[0])
    assert tmap[0] == 0 and depth[0, :8, 8:16].max() == 3001
    assert tmap[1] == np.float32(0.001).view(np.uint32)
    L = pkg._lib
    L.call("otx_slice_pretest", 0)
    try:
        with pytest.raises(Exception):
            staged(pkg, 64, 48, depth, color)
    finally:
        L.call("otx_slice_pretest", -1)


# ------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name,cfg,batch", [("small", SMALL, 16), ("small", SMALL, 3), ("tall", TALL, 16)])
def test_volume_parity(pkg, O, gpu, synth, hooks, name, cfg, batch, precision):
    """A 16-frame ring scan in 16-frame and 3-frame batches, in both staging forms: the oracle's volume and counters,
    and the same number of wave-frames dropped by the pre-test, above zero."""
    frames = as_frames(*ring(synth, cfg[0], 16))
    ref = oracle(O, ("ring16", name, True), cfg, frames)
    hooks(otx_slice_pretest=1, otx_integrate_fine=0)
    drops, exports = [], []
    for onepass in (-1, 0):
        hooks(otx_stage_onepass=onepass)
        vol = volume(pkg, cfg, batch=batch, precision=precision)
        integrate(pkg, vol, cfg, frames)
        compare(vol, ref)
        drops.append(dropped(pkg, vol))
        exports.append([t.cpu().numpy() for t in vol.export_units(color_dtype="float64")])
    assert drops[0] > 0, "the pre-test dropped no wave-frame"
    assert drops[0] == drops[1], "the two forms' maps drop different wave-frames"
    for a, b, what in zip(exports[0], exports[1], ("keys", "tsdf", "weight", "colour")):
        assert_bitwise(a, b, f"{what} of the two forms")


# ------------------------------------------------------------------------------------------------ 3. pool growth
@pytest.mark.gpu
@pytest.mark.parametrize("onepass", [-1, 0])
def test_pool_growth_replay_reads_the_first_pass_map(pkg, O, gpu, synth, hooks, onepass):
    """A 64-unit pool: the batch overflows it, the pool grows and the replay integrates the dropped units from the staged
    frames and the maps of the first pass: the oracle's volume, and the wave-frames dropped without growth."""
    frames = as_frames(*ring(synth, SMALL[0], 8))
    ref = oracle(O, ("ring8", "small", True), SMALL, frames)
    hooks(otx_slice_pretest=1, otx_integrate_fine=0, otx_stage_onepass=onepass)
    roomy = volume(pkg, SMALL)
    integrate(pkg, roomy, SMALL, frames)
    compare(roomy, ref)
    grown = volume(pkg, SMALL, max_units=64)
    integrate(pkg, grown, SMALL, frames)
    assert grown.num_units() > 64
    compare(grown, ref)
    assert dropped(pkg, roomy) > 0
    assert dropped(pkg, grown) == dropped(pkg, roomy)
