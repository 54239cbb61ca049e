"""Workgroup forms of the coarse integrate: one, two or four waves per workgroup (otx_integrate_workgroup), the
reciprocal table in dynamic LDS sized to the batch.  Every case is compared bitwise with the oracle through the facade
(unit keys, tsdf, weight, float64 colour; precision 32: colour at its existing 1e-4 tolerance) and by both counters,
for every form and both colour precisions.  The frames are tiny (64 x 48 pixels, 2-cm voxels, 32-cm units).

Two kinds of frames:
  site frames   a camera looking along +z from a translated origin, valid depth only in 3 x 3 pixel patches (or single
                pixels) placed so that every patch lies well inside one unit: a batch's unit count is chosen exactly;
  wall frames   a rendered wall, from a static camera or a short arc."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, assert_bitwise
from test_gpu_idle_frames import FORMS, HOOKS

INTR = (64, 48, 56.0, 56.0, 31.5, 23.5)
W, H = INTR[:2]
VOXEL, TRUNC = 0.02, 0.04
UNIT = 16 * VOXEL
RCP_N = 2048                      # csrc/tsdf_integrate.h: the table integrate serves frames since reset + the batch < RCP_N
WG_FORMS = (1, 2, 4)
PRECISIONS = (64, 32)
SITE_MM = 1120                    # depth of a site: z = 1.12 m, the middle of the units kz = 3
# pixels (multiples of the sampling stride) whose points at SITE_MM are 7-9 cm inside a unit: x = (u - 31.5) * 0.02
SITES = [(u, v) for v in (4, 20, 36) for u in (4, 20, 36, 52)]  # 12 units of one z layer
_cache = {}


# ------------------------------------------------------------------------------------------------------- frames
def _colour(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _translation(t):
    E = np.eye(4)
    E[:3, 3] = t
    return E


def site_frame(sites, seed, layer=0, patch=1):
    """depth SITE_MM in (2 * patch + 1)^2 pixels around each site, zero elsewhere; the camera moved by `layer` units
    along z, so the same pixels fall into the units of the z layer below (kz = 2)"""
    d = np.zeros((H, W), np.uint16)
    for u, v in sites:
        d[v - patch:v + patch + 1, u - patch:u + patch + 1] = SITE_MM
    return d, _colour(seed), _translation((0.0, 0.0, layer * UNIT))


def unit_count_batch(k):
    """a batch of two frames that touches exactly k <= 24 units: k sites dealt over two z layers"""
    a, b = SITES[:min(k, 12)], SITES[:max(k - 12, 0)]
    return [site_frame(a, 100 + k, 0), site_frame(b, 200 + k, 1)]


def wall_frames(synth, poses):
    if ("wall", poses) not in _cache:
        scene = synth.Scene(boxes=[synth.Box((-0.2, -3.0, 0.0), (0.0, 3.0, 3.0))], ring_radius=1.0, cam_height=0.9,
                            look_height=0.9, seed=5)
        out = []
        for i, k in enumerate(poses):
            T = synth.camera_pose(scene, k, 64)
            d, c = synth.render(scene, T, INTR, frame_id=i)
            out.append((d, c, np.linalg.inv(T)))
        _cache[("wall", poses)] = out
    return _cache[("wall", poses)]


# ------------------------------------------------------------------------------------------------------- both sides
def oracle(O, name, frames):
    """the oracle's volume after `frames` ((depth, colour, extrinsic) each), computed once per name and read-only"""
    if ("ref", name) not in _cache:
        ref = O.TSDF(VOXEL, TRUNC, 1, 4)
        for d, c, e in frames:
            ref.integrate(O.depth_to_float(d, 1000.0, 3.0), c, INTR, e)
        out = ref.export() + (ref.total_updates(), ref.unit_integrations())
        for a in out[:4]:
            a.setflags(write=False)
        _cache[("ref", name)] = out
    return _cache[("ref", name)]


def volume(pkg, batch, precision):
    integ = pkg.pipelines.integration
    return integ.ScalableTSDFVolume(voxel_length=VOXEL, sdf_trunc=TRUNC, color_type=integ.TSDFVolumeColorType.RGB8,
                                    batch_frames=batch, color_precision=precision)


def rgbd(pkg, d, c):
    return pkg.geometry.RGBDImage.create_from_color_and_depth(
        pkg.geometry.Image(c), pkg.geometry.Image(d), depth_scale=1000.0, depth_trunc=3.0,
        convert_rgb_to_intensity=False)


def integrate(pkg, vol, frames):
    intr = pkg.camera.PinholeCameraIntrinsic(*INTR)
    for d, c, e in frames:
        vol.integrate(rgbd(pkg, d, c), intr, e)


def compare_arrays(got, ref, precision, what=""):
    keys, tsdf, weight, col = got
    assert_bitwise(keys, ref[0], what + "unit keys")
    assert_bitwise(weight, ref[2], what + "voxel weights")
    assert_bitwise(tsdf, ref[1], what + "voxel tsdf")
    if precision == 64:
        assert_bitwise(col, ref[3], what + "voxel colours (float64)")
    else:
        np.testing.assert_allclose(col, ref[3], rtol=1e-4, atol=1e-4 * 255)


def compare(vol, ref, what=""):
    compare_arrays([t.cpu().numpy() for t in vol.export_units(color_dtype="float64")], ref, vol.color_precision, what)
    upd, units = vol.counters()
    assert upd == ref[4], what + "voxel updates"
    assert units == ref[5], what + "unit integrations"


class forced:
    """the workgroup form (and any of the existing hooks) forced for a block"""

    def __init__(self, pkg, wg, **hooks):
        self.L, self.wg, self.hooks = pkg._lib, wg, hooks

    def __enter__(self):
        self.L.call("otx_integrate_workgroup", self.wg)
        for hook, value in self.hooks.items():
            self.L.call(hook, value)

    def __exit__(self, *exc):
        self.L.call("otx_integrate_workgroup", -1)
        for hook in HOOKS:
            self.L.call(hook, -1)


forms = pytest.mark.parametrize("wg", WG_FORMS)
precisions = pytest.mark.parametrize("precision", PRECISIONS)


# ------------------------------------------------------------------------------------------------------- cases
def test_site_batches_have_the_unit_counts(O):
    """On the oracle alone: the site batches touch exactly 1, 7, 8, 9 and 17 units."""
    for k in (1, 7, 8, 9, 17):
        assert oracle(O, ("count", k), unit_count_batch(k))[0].shape[0] == k


@pytest.mark.gpu
@forms
@precisions
def test_partial_groups(pkg, O, gpu, precision, wg):
    """Batches of 1, 7, 8, 9 and 17 units: work lists that end inside a group of 8 units, at one and beyond it, so
    workgroups past the list's end leave (u >= n) and a unit's parts sit 8 items apart at every part count.  Each batch
    twice into its volume: fresh units, then units with state."""
    with forced(pkg, wg, otx_integrate_fine=0):
        for k in (1, 7, 8, 9, 17):
            frames = unit_count_batch(k) * 2
            vol = volume(pkg, 2, precision)
            integrate(pkg, vol, frames)
            compare(vol, oracle(O, ("count2", k), frames), f"{k} units: ")


@pytest.mark.gpu
@forms
@precisions
def test_table_grows_across_launches(pkg, O, gpu, synth, precision, wg):
    """set_batch(4) over 12 frames of an arc: rcp_hi is 4, 8, 12, so every launch asks for another LDS size."""
    frames = wall_frames(synth, (-3, -2, -1, 0, 1, 2, 3, 2, 1, 0, -1, -2))
    with forced(pkg, wg, otx_integrate_fine=0):
        vol = volume(pkg, 64, precision)
        vol.set_batch(4)
        integrate(pkg, vol, frames)
        compare(vol, oracle(O, "arc", frames))


@pytest.mark.gpu
@forms
@precisions
def test_last_table_entry(pkg, O, gpu, synth, precision, wg):
    """A static camera, 8 frames in batches of 4: the voxels seen by every frame reach weight 8 = frames since reset +
    the batch, so the last update of each batch reads the last entry the workgroup copied."""
    frames = wall_frames(synth, (0,)) * 8
    ref = oracle(O, "static8", frames)
    assert ref[2].max() == 8
    with forced(pkg, wg, otx_integrate_fine=0):
        vol = volume(pkg, 4, precision)
        integrate(pkg, vol, frames)
        compare(vol, ref)


def _long_static(synth):
    """the static wall frame, and a ramp frame: the same frame with all but a patch of its depth removed (few units, so
    two thousand of them are cheap on the oracle too)"""
    d, c, e = wall_frames(synth, (0,))[0]
    ramp = np.zeros_like(d)
    ramp[20:28, 28:36] = d[20:28, 28:36]
    return (d, c, e), (ramp, c, e)


@pytest.mark.gpu
@forms
@precisions
def test_switch_to_ieee_kernel(pkg, O, gpu, synth, precision, wg):
    """The same at the end of the table.  2043 ramp frames in batches of 64, then the whole frame: a batch of 4 to 2047
    frames (the last launch of the table kernel, rcp_hi = RCP_N - 1: the whole table but one entry in LDS, its last
    copied entry read by the voxels of the ramp's patch), a batch of 1 to 2048 (rcp_hi = RCP_N: the IEEE-division
    kernel), and a batch of 4 further."""
    full, ramp = _long_static(synth)
    n_ramp = RCP_N - 5
    frames = [ramp] * n_ramp + [full] * 9
    ref = oracle(O, "long", frames)
    assert ref[2].max() == n_ramp + 9
    intr = pkg.camera.PinholeCameraIntrinsic(*INTR)
    with forced(pkg, wg, otx_integrate_fine=0):
        vol = volume(pkg, 64, precision)
        image = rgbd(pkg, ramp[0], ramp[1])
        for _ in range(n_ramp):
            vol.integrate(image, intr, ramp[2])
        vol.flush()
        for batch in (4, 1, 4):
            vol.set_batch(batch)
            integrate(pkg, vol, [full] * batch)
            vol.flush()
        compare(vol, ref)


def _order_frames():
    """Two batches of 4 frames around the unit U = (0, 0, 3).  A patch in the middle of U updates it (frames 0, 2, 3, 4,
    6, 7, other colours each); frames 1 and 5 hold a single pixel whose point lies 3 cm outside U's -x face: within the
    truncation distance, so U is touched and the frame is in U's mask, but U's voxels project at least two pixels to the
    right of it, onto zero depth, and no wave of U updates.  That pixel's own unit V = (-1, 0, 3) is fresh in the first
    batch beside U; frame 5 looks from one unit further on, so its units (kz = 2) are fresh in the second batch."""
    mid = [(40, 32)]  # x = 0.17, y = 0.17: the middle of U
    out = []
    for i in range(8):
        if i in (1, 5):
            d, c, _ = site_frame([(32, 24)], 300 + i, patch=0)
            out.append((d, c, _translation((0.04, -0.15, (i == 5) * UNIT))))
        else:
            out.append(site_frame(mid, 300 + i, patch=2))
    return out


def test_order_scene_has_an_idle_touched_unit(O):
    """On the oracle alone: frame 1 touches U = (0, 0, 3) and V = (-1, 0, 3) and updates no voxel of U."""
    keys, _, weight = oracle(O, "order1", _order_frames()[1:2])[:3]
    assert keys.tolist() == [[-1, 0, 3], [0, 0, 3]]
    assert weight[0].max() == 1 and weight[1].max() == 0


@pytest.mark.gpu
@forms
@precisions
def test_order_per_voxel(pkg, O, gpu, precision, wg):
    """A unit whose mask has frames that no wave updates, between frames that do, with fresh units in the same batch:
    the state and the update count are the oracle's."""
    frames = _order_frames()
    with forced(pkg, wg, otx_integrate_fine=0):
        vol = volume(pkg, 4, precision)
        integrate(pkg, vol, frames)
        compare(vol, oracle(O, "order", frames))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["deferred_coarse", "deferred_fine"])
@precisions
def test_sharded_deferred_forms(pkg, O, gpu, synth, precision, form):
    """The fine slices keep four waves but take their table from the launch's dynamic LDS too: a volume sharded over two
    ranks, 12 frames in batches of 4 with the deferred integrate forced (two fused launches and a flush per rank),
    coarse and fine slices; the union of the ranks' units is the oracle's volume."""
    frames = wall_frames(synth, (-3, -2, -1, 0, 1, 2, 3, 2, 1, 0, -1, -2))
    ref = oracle(O, "arc", frames)
    parts = []
    with forced(pkg, -1, **FORMS[form]):
        for rank in range(2):
            vol = volume(pkg, 4, precision)
            vol.set_shard(rank, 2)
            integrate(pkg, vol, frames)
            parts.append([t.cpu().numpy() for t in vol.export_units(color_dtype="float64")])
    assert min(p[0].shape[0] for p in parts) > 0
    keys = np.concatenate([p[0] for p in parts])
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    compare_arrays([np.concatenate([p[i] for p in parts])[order] for i in range(4)], ref, precision)


CHILD = r"""
import importlib, sys, threading
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module(sys.argv[2])
data = np.load(sys.argv[3])
integ = pkg.pipelines.integration
torch.cuda.set_device(0)
intr = pkg.camera.PinholeCameraIntrinsic(*[float(x) if i > 1 else int(x) for i, x in enumerate(data["intr"])])
vols = [integ.ScalableTSDFVolume(voxel_length=float(data["voxel"]), sdf_trunc=float(data["trunc"]),
                                 color_type=integ.TSDFVolumeColorType.RGB8, batch_frames=4) for _ in range(2)]
streams = [torch.cuda.Stream() for _ in range(2)]
gate = threading.Barrier(2)
out, err = [None, None], []
def work(i):
    try:
        with torch.cuda.stream(streams[i]):
            gate.wait()
            for d, c, e in zip(data["depth"], data["color"], data["ext"]):
                im = pkg.geometry.RGBDImage.create_from_color_and_depth(
                    pkg.geometry.Image(c), pkg.geometry.Image(d), depth_scale=1000.0, depth_trunc=3.0,
                    convert_rgb_to_intensity=False)
                vols[i].integrate(im, intr, e)
            out[i] = [t.cpu().numpy() for t in vols[i].export_units(color_dtype="float64")] + list(vols[i].counters())
    except BaseException as ex:
        err.append(repr(ex))
        gate.abort()
threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
[t.start() for t in threads]
[t.join() for t in threads]
assert not err, err
np.savez(sys.argv[4], **{f"v{i}_{j}": np.asarray(a) for i in range(2) for j, a in enumerate(out[i])})
"""


@pytest.mark.gpu
def test_two_threads_first_integrate(pkg, O, gpu, synth, tmp_path):
    """The first integrates of a process under concurrency (the launch form and its occupancy are looked up and cached
    per device then), in a process of its own: two volumes created before either has integrated, then integrated at
    once by two host threads on two streams."""
    frames = wall_frames(synth, (-3, -2, -1, 0, 1, 2, 3, 2, 1, 0, -1, -2))
    ref = oracle(O, "arc", frames)
    src, dst = tmp_path / "frames.npz", tmp_path / "volumes.npz"
    np.savez(src, intr=np.asarray(INTR, np.float64), voxel=VOXEL, trunc=TRUNC, depth=np.stack([f[0] for f in frames]),
             color=np.stack([f[1] for f in frames]), ext=np.stack([f[2] for f in frames]))
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT, PKG, str(src), str(dst)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(dst)
    for i in range(2):
        compare_arrays([got[f"v{i}_{j}"] for j in range(4)], ref, 64, f"volume {i}: ")
        assert (int(got[f"v{i}_4"]), int(got[f"v{i}_5"])) == ref[4:], f"volume {i}: counters"
