"""Time cluster_dbscan against remove_radius_outlier on the same cloud in the same run: 100 000 points from
sample_points_uniformly of a synthetic object mesh (the four sides and the top of object 1's box), eps = radius = 0.02,
min_points = nb_points = 10.

Both are called through the C ABI on buffers allocated beforehand, each between two events on the stream (the calls end
in a synchronise, so the span is the call as its caller sees it): 2 warm-ups, median of 10.  ROR is one grid build
and one neighbourhood sweep; DBSCAN is the same grid build, three sweeps and the hooking, so the ratio says what the
clustering costs beyond a radius search.  Writes profiles/dbscan.json and prints it as the last line.  For per-kernel
times run it under `rocprofv3 --kernel-trace --stats -- python3 tools/dbscan_time.py --reps 3`."""
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
ap.add_argument("--eps", type=float, default=0.02)
ap.add_argument("--min-points", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan.json"))
a = ap.parse_args()

import torch

assert torch.cuda.is_available(), "dbscan_time.py needs a HIP device"
o3d = importlib.import_module(PKG)
synth = importlib.import_module(PKG + ".synth")
D, L = o3d._device, o3d._lib

box = synth.object_scene(1).boxes[0]
lo, hi = np.array(box.lo), np.array(box.hi)
V = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
Q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (1, 5, 7, 3)]  # the faces a scan sees
Tm = np.array([t for q in Q for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(V), o3d.utility.Vector3iVector(Tm))
cloud = mesh.sample_points_uniformly(a.points, seed=7)
xyz = cloud._xyz.dev()
n = int(xyz.shape[0])
labels, idx = D.empty((n,), "int32"), D.empty((n,), "int64")
n_clusters, n_kept = C.c_int32(0), C.c_int64(0)


def dbscan():
    L.call("ot_cluster_dbscan", D.ptr(xyz), n, a.eps, a.min_points, D.ptr(labels), C.byref(n_clusters),
           D.stream_ptr())


def ror():
    L.call("ot_remove_radius_outlier", D.ptr(xyz), n, a.min_points, a.eps, D.ptr(idx), C.byref(n_kept),
           D.stream_ptr())


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


out = {"dbscan_time": True, "n_points": n, "eps": a.eps, "min_points": a.min_points, "reps": a.reps,
       "warmup": a.warmup}
out["ot_remove_radius_outlier"] = timed(ror)
out["ot_cluster_dbscan"] = timed(dbscan)
out["ot_remove_radius_outlier_again"] = timed(ror)  # the yardstick before and after: drift of the machine
lab = D.to_host(labels)
out.update({"ratio_dbscan_over_ror": out["ot_cluster_dbscan"]["median_ms"] /
            out["ot_remove_radius_outlier"]["median_ms"],
            "n_clusters": int(n_clusters.value), "noise_points": int((lab == -1).sum()), "ror_kept": int(n_kept.value),
            "extent": (hi - lo).tolist(), "source_hash": L.source_hash()})
for k in ("ot_remove_radius_outlier", "ot_cluster_dbscan", "ot_remove_radius_outlier_again"):
    print(f"{k}: {out[k]['median_ms']:.3f} ms ({out[k]['min_ms']:.3f}-{out[k]['max_ms']:.3f})", flush=True)
print(f"cluster_dbscan / remove_radius_outlier = {out['ratio_dbscan_over_ror']:.2f}", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
