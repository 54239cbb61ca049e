"""bench.py as a plain run: `--gpus 1 --steps K --warmup W` times the headline only (every secondary leg is null without
--full), and --dump-outputs DIR writes the volume its last timed step left.  One short run of the real entry point on
an 8-frame scan; the dumped arrays are bit-exact against the CPU oracle's volume of the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bitwise

pytestmark = pytest.mark.gpu

FRAMES = 8
FULL_ONLY = ("roofline", "cpu_baseline", "sustained", "color32", "spatial_amdahl", "filtered", "objects", "hybrid_map",
             "single_frame", "spatial")


def test_plain_run_dumps_last_step(tmp_path, O, synth, gpu):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", str(FRAMES), "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["metric"] and line["dtype"]
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: frames of one step over the milliseconds one step took
    assert line["value"] == pytest.approx(FRAMES * 1e3 / line["ms_per_step"], rel=1e-2)
    for key in FULL_ONLY:
        assert line[key] is None, key

    got = {n: np.load(out / (n + ".npy")) for n in ("unit_keys", "unit_sums", "sample_units", "tsdf", "weight", "color")}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in got)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    depth, color, ext = synth.make_sequence(synth.Scene(seed=0), n_frames=FRAMES, intr=synth.REF_INTRINSICS_640)
    ref = O.TSDF(0.005, 0.04, 1, 4)
    for k in range(FRAMES):
        ref.integrate(O.depth_to_float(depth[k], 1000.0, 3.0), color[k], synth.REF_INTRINSICS_640, ext[k])
    rk, rt, rw, rc = ref.export()
    U = rk.shape[0]
    assert line["config"]["volume_units"] == U > 256  # more units than the sample: the sampled path is the one checked
    assert_bitwise(got["unit_keys"], rk.astype(np.float64), "dumped unit keys")
    pick = got["sample_units"].astype(np.int64)
    assert pick.shape == (256,) and (np.diff(pick) > 0).all() and 0 <= pick[0] and pick[-1] < U
    assert_bitwise(got["tsdf"], rt[pick], "dumped tsdf")
    assert_bitwise(got["weight"], rw[pick], "dumped weights")
    assert_bitwise(got["color"], rc[pick], "dumped float64 colours")
    # per-unit float64 sums over 4096 voxels: the weights are small integers (exact in any order); tsdf and colour sums
    # differ from numpy's by the summation order only, <= 4096 * 2^-53 relative to the sum of magnitudes
    assert_bitwise(got["unit_sums"][:, 1], rw.sum(1, dtype=np.float64), "per-unit weight sums")
    tol = 4096 * 2.0 ** -53
    mag_t = np.abs(rt).sum(1, dtype=np.float64)
    assert (np.abs(got["unit_sums"][:, 0] - rt.sum(1, dtype=np.float64)) <= tol * mag_t).all()
    assert (np.abs(got["unit_sums"][:, 2:] - rc.sum(1)) <= tol * np.abs(rc).sum(1)).all()
