"""Time PointCloud.segment_plane on a 100 000-point object cloud (synth.object_cloud: the four sides and the top of a
box, about a fifth of the points on each, so the loop never breaks early) with num_iterations 100 and 1 000,
distance_threshold 0.01.

The call goes through the C ABI on buffers allocated beforehand, between two events on the stream (it ends in a
synchronise, so the span is the call as its caller sees it): 2 warm-ups, median of 10.  The library's profile hook
(otx_segment_plane_profile) splits the last call: the counting kernels (events around each), the loop's wall time (the
rest of it is the round trips of the replay: candidates kernel, mail, host replay), the rmse tie-break, the refit's
chains (events) and the whole final pass (compaction, gather, chains, copies).  The 1 000-iteration call is repeated
with other chunk sizes (otx_segment_plane_chunk).  Writes profiles/segment_plane.json and prints it as the last line."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "object-triggered-3d-slam_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=100000)
ap.add_argument("--threshold", type=float, default=0.01)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_plane.json"))
a = ap.parse_args()

import torch

assert torch.cuda.is_available(), "segment_plane_time.py needs a HIP device"
o3d = importlib.import_module(PKG)
synth = importlib.import_module(PKG + ".synth")
D, L = o3d._device, o3d._lib

pts = synth.object_cloud(1, int(a.points * 1.05))[:a.points]
xyz = D.to_device(np.ascontiguousarray(pts, np.float64))
n = int(xyz.shape[0])
idx = D.empty((n,), "int64")
plane = np.zeros(4)
k, ev = C.c_int64(0), C.c_int32(0)
prof = (C.c_double * 8)()
NAMES = ("count_kernels_ms", "loop_wall_ms", "tie_break_wall_ms", "refit_chains_ms", "final_pass_wall_ms", "chunks",
         "holders", "evaluated")


def run(iters):
    L.call("ot_segment_plane", D.ptr(xyz), n, a.threshold, 3, iters, 0.99999999, 11,
           plane.ctypes.data_as(C.c_void_p), D.ptr(idx), C.byref(k), C.byref(ev), D.stream_ptr())


def timed(iters, chunk):
    lib = L.load()
    assert lib.otx_segment_plane_chunk(chunk) == 0
    lib.otx_segment_plane_profile(0, None)
    for _ in range(a.warmup):
        run(iters)
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(iters)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    res = {"num_iterations": iters, "chunk": chunk or 256, "median_ms": float(np.median(ts)),
           "min_ms": float(ts.min()), "max_ms": float(ts.max())}
    lib.otx_segment_plane_profile(1, None)  # the stages of one more call, with events between its kernels
    rows = []
    for _ in range(5):
        run(iters)
        lib.otx_segment_plane_profile(1, prof)
        rows.append(list(prof))
    lib.otx_segment_plane_profile(0, None)
    med = np.median(np.array(rows), axis=0)
    res["stages"] = {nm: float(v) for nm, v in zip(NAMES, med)}
    res["stages"]["replay_round_trips_ms"] = res["stages"]["loop_wall_ms"] - res["stages"]["count_kernels_ms"]
    res["n_inliers"], res["plane"] = int(k.value), plane.tolist()
    lib.otx_segment_plane_chunk(0)
    return res


out = {"segment_plane_time": True, "n_points": n, "distance_threshold": a.threshold, "ransac_n": 3, "reps": a.reps,
       "warmup": a.warmup, "runs": []}
for iters, chunk in ((100, 0), (1000, 0), (1000, 128), (1000, 512), (1000, 1024), (100, 0)):
    r = timed(iters, chunk)
    out["runs"].append(r)
    s = r["stages"]
    print(f"iterations {iters}, chunk {r['chunk']}: {r['median_ms']:.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}); "
          f"count kernels {s['count_kernels_ms']:.3f}, round trips {s['replay_round_trips_ms']:.3f}, tie-break "
          f"{s['tie_break_wall_ms']:.3f}, final pass {s['final_pass_wall_ms']:.3f} (refit chains "
          f"{s['refit_chains_ms']:.3f}); {int(s['chunks'])} chunks, {int(s['evaluated'])} counted", flush=True)
out["source_hash"] = L.source_hash()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
