"""Time the volume's three extractors on the configs[1] volume (256 frames of 640x480, 5 mm voxels, RGB8, seed 0).

extract_triangle_mesh(), extract_point_cloud() and extract_voxel_point_cloud() are called through the facade, each
between two events on the stream with the device idle before the first (the span is the call as its caller sees it:
the count's launches, its read-back, the allocation of the outputs and the emission): 3 warm-ups, median of 15.
Writes profiles/tsdf_cloud_time.json and prints it as the last line."""
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
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_cloud_time.json"))
a = ap.parse_args()

synth = importlib.import_module(PKG + ".synth")
# rendered by forked workers before this process touches the GPU
depth, color, ext = synth.make_sequence_parallel(synth.Scene(seed=0), n_frames=a.frames, intr=synth.REF_INTRINSICS_640)

import torch

assert torch.cuda.is_available(), "tsdf_cloud_time.py needs a HIP device"
torch.cuda.set_device(0)
o3d = importlib.import_module(PKG)
L = o3d._lib
lib = L.load()
integ = o3d.pipelines.integration
intr_t = synth.REF_INTRINSICS_640
W, H = intr_t[0], intr_t[1]
d_depth = torch.from_numpy(depth.view(np.int16)).cuda().view(torch.uint16).contiguous()
d_color = torch.from_numpy(color).cuda().contiguous()
ext = np.ascontiguousarray(ext, dtype=np.float64)
intr = L.ot_intrinsics(W, H, *intr_t[2:])
vol = integ.ScalableTSDFVolume(voxel_length=a.voxel, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for k in range(a.frames):
    st = lib.ot_tsdf_integrate_u16(vol._h, C.c_void_p(d_depth.data_ptr() + k * W * H * 2),
                                   C.c_void_p(d_color.data_ptr() + k * W * H * 3), C.byref(intr),
                                   ext[k].ctypes.data_as(C.c_void_p), 1000.0, 3.0, stream)
    if st:
        raise RuntimeError(lib.ot_last_error().decode())
vol.flush()
torch.cuda.synchronize()


def timed(fn):
    ts, res = [], None
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return res, {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


out = {"tsdf_cloud_time": True, "frames": a.frames, "voxel_length": a.voxel, "units": vol.num_units(),
       "reps": a.reps, "warmup": a.warmup}
mesh, out["extract_triangle_mesh"] = timed(vol.extract_triangle_mesh)
out["extract_triangle_mesh"].update(vertices=len(mesh.vertices), triangles=len(mesh.triangles))
cloud, out["extract_point_cloud"] = timed(vol.extract_point_cloud)
out["extract_point_cloud"]["points"] = len(cloud)
vox, out["extract_voxel_point_cloud"] = timed(vol.extract_voxel_point_cloud)
out["extract_voxel_point_cloud"]["points"] = len(vox)
out["source_hash"] = L.source_hash()
for k in ("extract_triangle_mesh", "extract_point_cloud", "extract_voxel_point_cloud"):
    print(f"{k}: {out[k]['median_ms']:.3f} ms ({out[k]['min_ms']:.3f}-{out[k]['max_ms']:.3f})", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
