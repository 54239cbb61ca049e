"""The slice pre-test's bound (csrc/slice_pretest.h) against brute force, on the CPU.  A stand-alone host program
(tests/slice_pretest_check.cpp, built here with the system compiler around the same header the integrate kernel
includes) decides every (unit, slice, frame) twice: by the header -- bounding box of the slice's voxel centres in the
image, tile-max depth map -- and by taking all 256 voxel centres of the slice through the integrate's float32 steps
and Open3D's projection and candidate test.  The header may never call a slice idle that has a candidate; and on five
frames of the headline scan it must drop at least 0.20 of the wave-frames (the model it was designed on gives 0.24 at
8-pixel tiles and a 6 x 6 cap), so the test cannot pass on a bound that drops nothing."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

TRUNC = 0.04
HEADLINE_FRAMES = (0, 40, 97, 150, 211)
WIDE_INTR = (64, 48, 32.0, 32.0, 31.5, 23.5)  # the 90-degree camera of tests/test_stage_record_bound.py
SIZES = {  # intrinsics, voxel length
    "640x480": ((640, 480, 565.6009, 565.6009, 320.5, 240.5), 0.005),
    "324x243": ((324, 243, 286.3, 286.3, 162.2, 121.7), 0.005),
    "37x29": ((37, 29, 33.0, 31.0, 18.5, 14.5), 0.01),
    "wide": (WIDE_INTR, 0.02),
}


# ----------------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("slice_pretest") / "slice_pretest_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, PKG, "csrc"),
                    os.path.join(ROOT, "tests", "slice_pretest_check.cpp"), "-o", str(exe)], check=True)

    def run(cases, path):
        with open(path, "wb") as f:
            for intr, vl, ext, depth, keys in cases:
                w, h, fx, fy, cx, cy = intr
                depth = np.ascontiguousarray(depth, np.float32)
                keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
                assert depth.shape == (h, w)
                vlf = np.float32(vl)  # (float)(unit_length / 16)
                f.write(struct.pack("<ii4ffdfi", w, h, fx, fy, cx, cy, float(vlf), 16.0 * vl, TRUNC, keys.shape[0]))
                f.write(np.asarray(ext, np.float64)[:3].astype(np.float32).tobytes())
                f.write(depth.tobytes())
                f.write(keys.tobytes())
        out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
        rows = np.array([[int(x) for x in line.split()] for line in out if line.strip()], np.int64).reshape(-1, 4)
        assert rows.shape[0] == len(cases)
        return rows  # per case: wave-frames, dropped, idle by brute force, dropped with a candidate

    return run


# ----------------------------------------------------------------------------------------------------- inputs
def staged(depth_u16, scale=1000.0, trunc=3.0):
    """Image::ConvertDepthToFloatImage: float32 division, the truncation compared in float64"""
    f = depth_u16.astype(np.float32) / np.float32(scale)
    f[f.astype(np.float64) >= trunc] = 0.0
    return f


def touched_units(depth, intr, ext, unit_len, stride=4):
    """Open3D's touch: stride samples unprojected in float64, units of [p - trunc, p + trunc] per axis"""
    w, h, fx, fy, cx, cy = intr
    rr, cc = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    z = depth[rr, cc].astype(np.float64)
    ok = z > 0
    z, rr, cc = z[ok], rr[ok], cc[ok]
    p = np.stack([(cc - cx) * z / fx, (rr - cy) * z / fy, z, np.ones_like(z)], 1) @ np.linalg.inv(ext).T
    lo = np.floor((p[:, :3] - TRUNC) / unit_len).astype(np.int64)
    hi = np.floor((p[:, :3] + TRUNC) / unit_len).astype(np.int64)
    span = int((hi - lo).max())
    keys = []
    for dx in range(span + 1):
        for dy in range(span + 1):
            for dz in range(span + 1):
                k = lo + np.array([dx, dy, dz])
                keys.append(k[(k <= hi).all(1)])
    return np.unique(np.concatenate(keys), axis=0)


def cube_of_units(centre, unit_len, radius):
    """every unit within `radius` units of the unit that holds `centre`: in front of the camera, behind it, around it"""
    c = np.floor(np.asarray(centre) / unit_len).astype(np.int64)
    r = np.arange(-radius, radius + 1)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return g + c


def random_extrinsic(rng, reach):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-reach, reach, 3)
    return np.linalg.inv(T), T[:3, 3]


def adversarial_depth(rng, w, h, near, kind):
    """a noisy plane at `near` metres with dropout, an all-zero tile, one far pixel inside a near tile; kind "float":
    float depths holding negatives, NaN and +inf as well"""
    d = (near + 0.02 * rng.standard_normal((h, w))).astype(np.float32)
    d[rng.random((h, w)) < 0.05] = 0.0
    d[8:16, 8:16] = 0.0
    d[min(h - 1, 19), min(w - 1, 21)] = np.float32(near + 0.55)
    if kind == "float":
        m = rng.random((h, w))
        d[m < 0.03] = -1.0
        d[(m >= 0.03) & (m < 0.06)] = np.nan
        d[(m >= 0.06) & (m < 0.07)] = np.inf
    return d


# ----------------------------------------------------------------------------------------------------- cases
def test_headline_frames(checker, synth, tmp_path):
    """Five frames of the headline scan, the units each frame touches: nothing live is dropped, and at least a fifth of
    all wave-frames is."""
    intr, vl = SIZES["640x480"]
    depth, _, ext = synth.make_sequence(synth.Scene(seed=0), n_frames=256, intr=intr, frames=HEADLINE_FRAMES)
    cases = []
    for k in range(len(HEADLINE_FRAMES)):
        f = staged(depth[k])
        cases.append((intr, vl, ext[k], f, touched_units(f, intr, ext[k], 16.0 * vl)))
    rows = checker(cases, tmp_path / "headline.bin")
    total, dropped, idle, wrong = rows.sum(0)
    print(f"headline: {total} wave-frames, dropped {dropped / total:.4f}, idle {idle / total:.4f}")
    assert wrong == 0, f"{wrong} slices with a candidate were called idle: {rows.tolist()}"
    assert total > 50000
    assert dropped >= 0.20 * total, f"only {dropped / total:.4f} of the wave-frames dropped"


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["u16", "float"])
def test_random_poses(checker, tmp_path, size, kind):
    """Random cameras (any rotation) inside a cube of units: bricks a few centimetres from the camera, behind it,
    straddling z = 0 and every image border, under depth images with dropout, an empty tile, a far pixel in a near
    tile and (float depth) negatives, NaN and +inf."""
    intr, vl = SIZES[size]
    w, h = intr[:2]
    unit_len = 16.0 * vl
    rng = np.random.default_rng(list(SIZES).index(size) * 2 + (kind == "float"))
    cases = []
    for i in range(6):
        ext, pos = random_extrinsic(rng, 2.0 if i else 0.0)
        near = (5.0 + 2.0 * rng.random()) * unit_len
        d = adversarial_depth(rng, w, h, near, kind)
        cases.append((intr, vl, ext, d, cube_of_units(pos, unit_len, 8)))
    rows = checker(cases, tmp_path / "random.bin")
    total, dropped, idle, wrong = rows.sum(0)
    print(f"{size} {kind}: {total} wave-frames, dropped {dropped / total:.4f}, idle {idle / total:.4f}")
    assert wrong == 0, f"{wrong} slices with a candidate were called idle: {rows.tolist()}"
    assert 0 < idle < total and dropped > 0  # both kinds of slice were there, and the bound is not vacuous


def test_truncation_edge(checker, tmp_path):
    """Depth planes that put a slice's nearest voxel within an ulp on either side of d - z = -trunc: a camera looking
    along +z from the origin, so a voxel's camera z is its world z (float32: half a voxel, then adds of the voxel
    length), constant depth images at RN(z - trunc) and its neighbours."""
    intr, vl = SIZES["324x243"]
    w, h = intr[:2]
    vlf = np.float32(vl)
    t = np.float32(TRUNC)
    cases = []
    for kz in (3, 6, 11):
        for zq in range(4):
            z = np.float32(vlf * np.float32(0.5)) + np.float32(kz * 16.0 * vl)
            for _ in range(4 * zq):
                z = np.float32(z + vlf)
            d0 = np.float32(z - t)
            for d in (d0, np.nextafter(d0, np.float32(0)), np.nextafter(d0, np.float32(9)),
                      np.nextafter(np.nextafter(d0, np.float32(9)), np.float32(9))):
                keys = np.array([[0, 0, kz], [-1, 0, kz], [0, -1, kz], [-1, -1, kz]])
                cases.append((intr, vl, np.eye(4), np.full((h, w), d, np.float32), keys))
    rows = checker(cases, tmp_path / "edge.bin")
    total, dropped, idle, wrong = rows.sum(0)
    assert wrong == 0, f"{wrong} slices with a candidate were called idle: {rows.tolist()}"
    assert 0 < idle < total  # the planes do separate the slices
