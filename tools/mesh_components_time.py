"""Time the mesh clean-up recipe -- cluster_connected_triangles -> remove_triangles_by_mask (clusters smaller than
--min-triangles) -> remove_unreferenced_vertices -- on the marching-cubes mesh of the bench's object scan
(synth.object_scene(0), 64 frames at 640x480, 5 mm voxels, sdf_trunc 0.04), beside the same recipe in numpy (scipy's
connected_components when scipy is present) on the same arrays on the host.

The three C-ABI calls run on buffers allocated beforehand, each between two events on the stream (every call ends in a
synchronise, so the span is the call as its caller sees it); the facade recipe, downloads and the host-side mask
included, is timed the same way: 2 warm-ups, median of 10.  Writes profiles/mesh_components.json and prints it as the
last line.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python3
tools/mesh_components_time.py --reps 3 --no-host`."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "object-triggered-3d-slam_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--min-triangles", type=int, default=100)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components.json"))
a = ap.parse_args()

synth = importlib.import_module(PKG + ".synth")
depth, color, ext = synth.make_sequence_parallel(synth.object_scene(0), n_frames=a.frames)  # before the GPU is opened

import torch

assert torch.cuda.is_available(), "mesh_components_time.py needs a HIP device"
o3d = importlib.import_module(PKG)
D, L = o3d._device, o3d._lib
integ = o3d.pipelines.integration
intr = o3d.camera.PinholeCameraIntrinsic(*synth.REF_INTRINSICS_640)
vol = integ.ScalableTSDFVolume(voxel_length=a.voxel, sdf_trunc=0.04, color_type=integ.TSDFVolumeColorType.RGB8)
for k in range(depth.shape[0]):
    rgbd = o3d.geometry.RGBDImage.create_from_color_and_depth(
        o3d.geometry.Image(color[k]), o3d.geometry.Image(depth[k]), depth_scale=1000.0, depth_trunc=3.0,
        convert_rgb_to_intensity=False)
    vol.integrate(rgbd, intr, ext[k])
mesh = vol.extract_triangle_mesh()
V, VC, T = mesh._v.dev().clone(), mesh._vc.dev().clone(), mesh._t.dev().clone()
nv, nt = int(V.shape[0]), int(T.shape[0])
print(f"mesh: {nv} vertices, {nt} triangles", flush=True)

labels, counts = D.empty((nt,), "int32"), D.empty((nt,), "int32")
areas, mask = D.empty((nt,), "float64"), D.empty((nt,), "uint8")
T1, T2, kept = D.empty((nt, 3), "int32"), D.empty((nt, 3), "int32"), D.empty((nv,), "int32")
n_clusters, n_tri, n_vert = C.c_int64(0), C.c_int64(0), C.c_int64(0)


def cluster():
    L.call("ot_mesh_cluster_connected_triangles", D.ptr(T), nt, D.ptr(V), nv, D.ptr(labels), D.ptr(counts),
           D.ptr(areas), C.byref(n_clusters), D.stream_ptr())


def by_mask():
    L.call("ot_mesh_remove_triangles_by_mask", D.ptr(T), nt, D.ptr(mask), D.ptr(T1), C.byref(n_tri), D.stream_ptr())


def unreferenced():  # (the copy keeps the input of every repetition the same; it is inside the span)
    T2[:n_tri.value].copy_(T1[:n_tri.value])
    L.call("ot_mesh_remove_unreferenced_vertices", nv, D.ptr(T2), n_tri.value, D.ptr(kept), C.byref(n_vert),
           D.stream_ptr())


def facade():
    m = o3d.geometry.TriangleMesh()
    m._v, m._vc, m._t = (o3d.geometry._Arr(dev=x) for x in (V, VC, T))
    lab, cnt, _ = m.cluster_connected_triangles()
    small = np.asarray(cnt)[np.asarray(lab)] < a.min_triangles
    m.remove_triangles_by_mask(small)
    m.remove_unreferenced_vertices()
    return m


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


def host_recipe(Vh, Th):
    """the same recipe on the host: vectorised numpy, components by scipy when it is there"""
    e = np.sort(np.stack([Th[:, [0, 1]], Th[:, [1, 2]], Th[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1).astype(np.int64)
    key = (e[:, 0] << 32) | e[:, 1]
    order = np.argsort(key, kind="stable")
    sk, owner = key[order], order // 3
    same = np.nonzero(sk[1:] == sk[:-1])[0]
    p, q = owner[same], owner[same + 1]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        g = coo_matrix((np.ones(len(p), np.int8), (p, q)), shape=(len(Th), len(Th)))
        comp = connected_components(g, directed=False)[1]
        how = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        comp = np.arange(len(Th))
        while True:  # min-label propagation with pointer jumping
            new = comp.copy()
            m = np.minimum(comp[p], comp[q])
            np.minimum.at(new, p, m)
            np.minimum.at(new, q, m)
            new = new[new]
            if (new == comp).all():
                break
            comp = new
        how = "numpy min-label propagation"
    _, first, inv = np.unique(comp, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    lab = rank[inv]
    cnt = np.bincount(lab)
    p0, p1, p2 = Vh[Th[:, 0]], Vh[Th[:, 1]], Vh[Th[:, 2]]
    area = np.bincount(lab, weights=0.5 * np.linalg.norm(np.cross(p0 - p1, p0 - p2), axis=1))
    keep = cnt[lab] >= a.min_triangles
    Tk = Th[keep]
    used = np.zeros(len(Vh), bool)
    used[Tk.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return lab.astype(np.int32), cnt, area, Vh[used], new[Tk].astype(np.int32), how


out = {"mesh_components_time": True, "n_vertices": nv, "n_triangles": nt, "frames": a.frames, "voxel_length": a.voxel,
       "min_triangles": a.min_triangles, "reps": a.reps, "warmup": a.warmup}
out["ot_mesh_cluster_connected_triangles"] = timed(cluster)
mask.copy_((counts.to(torch.int64)[labels.to(torch.int64)] < a.min_triangles).to(torch.uint8))
out["ot_mesh_remove_triangles_by_mask"] = timed(by_mask)
out["ot_mesh_remove_unreferenced_vertices"] = timed(unreferenced)
out["facade_recipe"] = timed(facade)
res = facade()
cnt_d = D.to_host(counts[:n_clusters.value])
out.update({"n_clusters": int(n_clusters.value), "largest_clusters": sorted(cnt_d.tolist(), reverse=True)[:5],
            "triangles_kept": int(n_tri.value), "vertices_kept": int(n_vert.value),
            "three_calls_ms": sum(out[k]["median_ms"] for k in (
                "ot_mesh_cluster_connected_triangles", "ot_mesh_remove_triangles_by_mask",
                "ot_mesh_remove_unreferenced_vertices"))})
if not a.no_host:
    Vh, Th = D.to_host(V), D.to_host(T)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        lab_h, cnt_h, area_h, V2h, T2h, how = host_recipe(Vh, Th)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["host_numpy_recipe"] = {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)),
                                "components_by": how}
    same = (np.array_equal(lab_h, D.to_host(labels)) and np.array_equal(cnt_h, cnt_d) and
            np.array_equal(T2h, np.asarray(res.triangles)) and np.array_equal(V2h, np.asarray(res.vertices)))
    out["host_and_device_results_equal"] = bool(same)
    out["max_rel_area_difference"] = float(np.max(np.abs(area_h - D.to_host(areas[:n_clusters.value])) /
                                                  np.maximum(area_h, 1e-300)))
out["source_hash"] = L.source_hash()
for k, v in out.items():
    if isinstance(v, dict) and "median_ms" in v:
        print(f"{k}: {v['median_ms']:.3f} ms ({v['min_ms']:.3f}-{v['max_ms']:.3f})", flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
