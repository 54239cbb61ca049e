"""Projection edges of the integrate's frame loop.  The coarse loop certifies a voxel's fast projection, takes the image
bounds of a certified lane from its integer pixel, sends the unsure lanes through the exact quotients and Open3D's own
bound tests behind one wave-uniform branch, and lets every lane gather, the voxels outside the image from past the end
of the frame.  The scene and the intrinsics put voxel visits into every class that code treats differently:

  image-border slivers   visits whose exact u_f (v_f) lies in [0, 1e-4) -- case "low" -- or in [W - 1e-4, W)
                         ([H - 1e-4, H)) -- case "high": outside for Open3D, inside for a test on floor().  They are
                         constructed: one voxel centre of a touched unit, its quotient chain in float32 numpy in the
                         oracle's order, cx (cy) set so that the visit lands about 5e-5 inside the sliver, above a
                         pixel with a depth in the voxel's truncation band;
  near a pixel boundary  interior visits within proj_eps of an integer u_f or v_f (the exact path);
  behind the camera      a block of 6-cm depths in one frame: its units reach behind the camera plane;
  outside the image      wave-frames (8 x 8 columns x 4 z) that lie wholly beyond each of the four image sides;
  zero depth             a block of missing depth in some frames, under voxels that project into the image.

A CPU test counts the classes with the float32 restatement on the oracle's units (the units each frame touches: the
oracle's volume after that frame alone).  The GPU cases compare every instantiation of the integrate bitwise with the
oracle through the C ABI: unit keys, tsdf, weight, float64 colour and both counters (precision 32: colour at its
existing 1e-4 tolerance)."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bitwise
from test_gpu_idle_frames import FORMS, HOOKS

BASE = (160, 120, 80.0, 80.0, 79.5, 59.5)  # 90 x 74 degrees
W, H = BASE[:2]
VOXEL, TRUNC = 0.005, 0.04                 # 8-cm units
POSES = (-3, -2, -1, 0, 1, 2, 3, 0)        # ring positions of 64: +-17 degrees around the wall's normal
HOLED = (2, 3, 5)                          # frames with the block of zero depth
HOLE = (slice(35, 85), slice(50, 120))     # rows, columns
NEAR_FRAME = 6                             # the frame with the block of 6-cm depths
NEAR = (slice(50, 70), slice(70, 90))
NEAR_MM = 60
PIVOT = 7                                  # the frame whose visits the slivers are constructed on (no hole, no block)
CASES = ("low", "high")
F32 = np.float32
_cache = {}


def proj_eps(w, h):
    """the library's certification margin (csrc/tsdf.hip, integrate_params)"""
    return F32(np.ldexp(max(w, h) + 2.0, -21) + 1.2e-4)


def _frames(synth):
    """depth, colour and extrinsics of the 8 frames (rendered with BASE: the images are data, the same for both cases)"""
    if "frames" not in _cache:
        scene = synth.Scene(boxes=[synth.Box((-0.2, -3.0, 0.0), (0.0, 3.0, 3.0))], ring_radius=0.5, cam_height=0.9,
                            look_height=0.9, seed=11)
        dep, col, ext = [], [], []
        for i, k in enumerate(POSES):
            T = synth.camera_pose(scene, k, 64)
            d, c = synth.render(scene, T, BASE, frame_id=i)
            if i in HOLED:
                d[HOLE] = 0
            if i == NEAR_FRAME:
                d[NEAR] = NEAR_MM
            dep.append(d), col.append(c), ext.append(np.linalg.inv(T))
        _cache["frames"] = (np.stack(dep), np.stack(col), np.stack(ext))
    return _cache["frames"]


def _frame_units(O, synth, intr, f):
    """keys of the units frame f touches: the oracle's volume after that frame alone"""
    key = ("units", intr, f)
    if key not in _cache:
        depth, color, ext = _frames(synth)
        ref = O.TSDF(VOXEL, TRUNC, 1, 4)
        ref.integrate(O.depth_to_float(depth[f], 1000.0, 3.0), color[f], intr, ext[f])
        _cache[key] = ref.export()[0]
    return _cache[key]


def visits(intr, extrinsic, keys):
    """Open3D's projection of every voxel of the units `keys` in one frame, in float32 and the oracle's order of
    operations: (q_u, q_v, z), each [U][16 x][16 y][16 z] -- q the quotient (pc * f) / z, so u_f = (q_u + cx) + 0.5"""
    fx, fy = F32(intr[2]), F32(intr[3])
    E = np.asarray(extrinsic, np.float64).astype(F32)
    unit_len = VOXEL * 16.0
    vl = F32(unit_len / 16.0)
    half = vl * F32(0.5)
    o = (np.asarray(keys, np.float64) * unit_len).astype(F32)
    idx = np.arange(16, dtype=F32)
    px = ((half + vl * idx)[None, :] + o[:, 0:1])[:, :, None]
    py = ((half + vl * idx)[None, :] + o[:, 1:2])[:, None, :]
    pz = (half + o[:, 2])[:, None, None]
    pc = [((E[r, 0] * px + E[r, 1] * py) + E[r, 2] * pz) + E[r, 3] for r in range(3)]
    es = [E[r, 2] * vl for r in range(3)]
    out = np.empty((3,) + pc[0].shape + (16,), F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for z in range(16):
            out[0, ..., z] = (pc[0] * fx) / pc[2]
            out[1, ..., z] = (pc[1] * fy) / pc[2]
            out[2, ..., z] = pc[2]
            pc = [pc[r] + es[r] for r in range(3)]
    return out


def _uv(q, c):
    return (q + F32(c)) + F32(0.5)


def _place(q, size, side):
    """the float32 principal point c for which (q + c) + 0.5 lands about 5e-5 inside the sliver of `side`"""
    lo, hi = (2e-5, 8e-5) if side == "low" else (size - 8e-5, size - 2e-5)
    c = F32((lo + hi) / 2 - 0.5 - float(q))
    for _ in range(64):
        r = float(_uv(q, c))
        if lo <= r <= hi:
            return float(c)
        c = np.nextafter(c, F32(np.inf) if r < lo else F32(-np.inf))
    raise AssertionError("no principal point puts the visit into the sliver")


def intrinsics(O, synth, side):
    """BASE with cx and cy moved by less than a pixel, so that one visit of PIVOT lands in the u sliver of `side` and
    another in the v sliver, each above a pixel whose depth is within half the truncation distance of the voxel"""
    if ("intr", side) not in _cache:
        depth, _, ext = _frames(synth)
        d = O.depth_to_float(depth[PIVOT], 1000.0, 3.0)
        qu, qv, z = visits(BASE, ext[PIVOT], _frame_units(O, synth, BASE, PIVOT))
        with np.errstate(invalid="ignore"):
            u, v = _uv(qu, BASE[4]), _uv(qv, BASE[5])
            c = []
            for a, b, size, other, along in ((u, v, W, H, 1), (v, u, H, W, 0)):
                edge = 0.0 if side == "low" else float(size)
                m = (z > 0) & (np.abs(a - F32(edge)) < 0.4) & (b > 8) & (b < other - 8)
                pa = np.full(b.shape, 0 if side == "low" else size - 1)
                pb = np.clip(b, 0, other - 1).astype(np.int64)
                dd = d[pb, pa] if along else d[pa, pb]
                m &= (dd > 0) & (np.abs(dd - z) < TRUNC / 2)
                pick = np.argwhere(m)
                assert len(pick) > 0, "no voxel near the image border to place"
                q = (qu if along else qv)[tuple(pick[len(pick) // 2])]
                c.append(_place(q, size, side))
        _cache[("intr", side)] = BASE[:4] + (c[0], c[1])
    return _cache[("intr", side)]


def classes(O, synth, intr):
    """counts of the voxel visits (and wave-frames) of every class, on the units each frame touches"""
    depth, _, ext = _frames(synth)
    eps = proj_eps(W, H)
    safe_w, safe_h = F32(W) - F32(0.0001), F32(H) - F32(0.0001)
    m1 = F32(0.0001)
    n = dict.fromkeys(("u_low", "u_high", "v_low", "v_high", "near_boundary", "behind", "zero_depth", "left", "right",
                       "top", "bottom", "visits"), 0)
    for f in range(len(POSES)):
        d = O.depth_to_float(depth[f], 1000.0, 3.0)
        qu, qv, z = visits(intr, ext[f], _frame_units(O, synth, intr, f))
        with np.errstate(invalid="ignore"):
            u, v = _uv(qu, intr[4]), _uv(qv, intr[5])
            front = z > 0
            u_ok, v_ok = (u >= m1) & (u < safe_w), (v >= m1) & (v < safe_h)
            pu, pv = np.clip(u, 0, W - 1).astype(np.int64), np.clip(v, 0, H - 1).astype(np.int64)
            dd = d[pv, pu]
            band = (dd > 0) & (np.abs(dd - z) < F32(TRUNC))  # a wrongly accepted visit would update the voxel
            n["u_low"] += int((front & (u >= 0) & (u < m1) & v_ok & band).sum())
            n["u_high"] += int((front & (u >= safe_w) & (u < W) & v_ok & band).sum())
            n["v_low"] += int((front & (v >= 0) & (v < m1) & u_ok & band).sum())
            n["v_high"] += int((front & (v >= safe_h) & (v < H) & u_ok & band).sum())
            inside = front & (u >= 1) & (u < W - 1) & (v >= 1) & (v < H - 1)
            n["near_boundary"] += int((inside & ((np.abs(u - np.rint(u)) <= eps) | (np.abs(v - np.rint(v)) <= eps))).sum())
            n["behind"] += int((~front).sum())
            n["zero_depth"] += int((front & u_ok & v_ok & (dd == 0)).sum())
            # one coarse wave: 8 x 8 columns x 4 consecutive z
            wave = lambda m: int(m.reshape(-1, 2, 8, 2, 8, 4, 4).all(axis=(2, 4, 6)).sum())
            n["left"] += wave(front & (u < 0))
            n["right"] += wave(front & (u >= W))
            n["top"] += wave(front & (v < 0))
            n["bottom"] += wave(front & (v >= H))
            n["visits"] += u.size
    return n


@pytest.mark.parametrize("side", CASES)
def test_scene_covers_every_class(O, synth, side):
    """On the oracle alone: the scene and the intrinsics of each case put visits into every class."""
    intr = intrinsics(O, synth, side)
    assert abs(intr[4] - BASE[4]) < 1 and abs(intr[5] - BASE[5]) < 1
    n = classes(O, synth, intr)
    print(side, intr, n)
    assert n["u_" + side] >= 1 and n["v_" + side] >= 1, "image-border slivers"
    assert n["near_boundary"] >= 100
    assert n["behind"] >= 1
    assert n["zero_depth"] >= 1
    assert min(n["left"], n["right"], n["top"], n["bottom"]) >= 1, "wave-frames wholly outside the image on each side"


def _oracle(O, synth, side, lo, hi):
    """the oracle's volume after frames [lo, hi), computed once and shared (read-only)"""
    key = ("ref", side, lo, hi)
    if key not in _cache:
        depth, color, ext = _frames(synth)
        intr = intrinsics(O, synth, side)
        ref = O.TSDF(VOXEL, TRUNC, 1, 4)
        for k in range(lo, hi):
            ref.integrate(O.depth_to_float(depth[k], 1000.0, 3.0), color[k], intr, ext[k])
        out = ref.export() + (ref.total_updates(), ref.unit_integrations())
        for a in out[:4]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _volume(pkg, batch, precision=64):
    integ = pkg.pipelines.integration
    return integ.ScalableTSDFVolume(voxel_length=VOXEL, sdf_trunc=TRUNC, color_type=integ.TSDFVolumeColorType.RGB8,
                                    batch_frames=batch, color_precision=precision)


def _integrate(pkg, vol, intr_t, depth, color, ext, float_path=False):
    intr = pkg.camera.PinholeCameraIntrinsic(*intr_t)
    for k in range(depth.shape[0]):
        rgbd = pkg.geometry.RGBDImage.create_from_color_and_depth(
            pkg.geometry.Image(color[k]), pkg.geometry.Image(depth[k]), depth_scale=1000.0, depth_trunc=3.0,
            convert_rgb_to_intensity=False)
        if float_path:
            rgbd._raw_depth = None  # the float-depth entry point (ot_tsdf_integrate)
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


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("division", ["table", "ieee"])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("side", CASES)
def test_projection_edges_every_instantiation(pkg, O, gpu, synth, side, precision, division, form):
    """Both cases through every instantiation of the integrate (colour precision x division form x slice form), the
    8 frames in batches of 3.  table: a fresh volume.  ieee: volume A integrates the first 3 frames and exports, volume
    B imports A's units (arbitrary state: the IEEE-division kernels) and integrates the other 5 with the form forced;
    B's counters are the oracle's for all frames less those of the first 3."""
    depth, color, ext = _frames(synth)
    intr = intrinsics(O, synth, side)
    n = len(POSES)
    ref = _oracle(O, synth, side, 0, n)
    L = pkg._lib
    if division == "table":
        vol, first = _volume(pkg, 3, precision), 0
    else:
        a = _volume(pkg, None, precision)
        _integrate(pkg, a, intr, depth[:3], color[:3], ext[:3])
        vol, first = _volume(pkg, 3, precision), 3
        vol.import_units(*a.export_units())
        upd3, units3 = _oracle(O, synth, side, 0, 3)[4:]
        assert tuple(a.counters()) == (upd3, units3)
        ref = ref[:4] + (ref[4] - upd3, ref[5] - units3)
    try:
        for hook, value in FORMS[form].items():
            L.call(hook, value)
        _integrate(pkg, vol, intr, depth[first:], color[first:], ext[first:])
        _compare(vol, ref)
    finally:
        for hook in HOOKS:
            L.call(hook, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("side", CASES)
def test_projection_edges_float_depth(pkg, O, gpu, synth, side):
    """the float-depth entry point (ot_tsdf_integrate), batches of 3"""
    depth, color, ext = _frames(synth)
    vol = _volume(pkg, 3)
    _integrate(pkg, vol, intrinsics(O, synth, side), depth, color, ext, float_path=True)
    _compare(vol, _oracle(O, synth, side, 0, len(POSES)))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ot_tsdf_integrate_u16", "ot_tsdf_integrate"])
def test_frame_size_bound(pkg, gpu, entry):
    """A frame of 2^28 pixels or more is refused when it is queued (the gathers' 32-bit byte offsets and the pixel
    index of the voxels outside the image assume fewer): an error, no frame pending, no kernel launched."""
    import torch

    L = pkg._lib
    vol = _volume(pkg, 3)
    buf = torch.zeros(16, dtype=torch.uint8, device="cuda")  # never read: the sizes are checked first
    ext = np.eye(4)
    for w, h in ((1 << 14, 1 << 14), (1 << 28, 1), (1, 1 << 28)):
        intr = L.ot_intrinsics(w, h, 80.0, 80.0, 79.5, 59.5)
        args = (vol._h, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), C.byref(intr), ext.ctypes.data)
        with pytest.raises(L.OTError, match="2\\^28 pixels"):
            L.call(entry, *(args + ((1000.0, 3.0, None) if entry.endswith("u16") else (None,))))
    pending = C.c_int32(-1)
    L.call("ot_tsdf_pending_frames", vol._h, C.byref(pending))
    assert pending.value == 0
    assert tuple(vol.counters()) == (0, 0)
