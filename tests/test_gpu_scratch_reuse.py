"""The operators' scratch buffers (csrc/scratch_slots.h) under reuse and growth.  On one host thread and one stream, ten
operators run on seeded clouds of 300 to 3000 points in a fixed order (round 1), again in reverse order on clouds twice
the size -- so every buffer grows, and is freed and reallocated, while the others still hold what the previous operator
left -- (round 2), and again at the first sizes (round 3).  Rounds 1 and 3 must agree bit for bit operator by operator
(a buffer that outgrew its first size serves the small call unchanged), and round 2 must agree bit for bit with the
same calls made first thing in a fresh child process (every buffer allocated at that size from scratch: nothing an
earlier operator left in a shared or a regrown buffer reaches a result).  The allocation count after the three rounds
is printed (a change of it between two builds means a buffer was merged, split or sized differently)."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, assert_bitwise


def cloud(seed, n):
    """a noisy plane, a blob above it and a few far outliers: every operator below has something to find"""
    rng = np.random.default_rng(seed)
    k = n // 10
    plane = np.column_stack([rng.uniform(-1, 1, n - 2 * k), rng.uniform(-1, 1, n - 2 * k),
                             0.004 * rng.standard_normal(n - 2 * k)])
    blob = np.array([0.3, -0.2, 0.5]) + 0.08 * rng.standard_normal((k, 3))
    far = rng.uniform(-3, 3, (k, 3))
    p = np.concatenate([plane, blob, far])
    return np.ascontiguousarray(p[rng.permutation(n)])


def sheets(k):
    """two separate k x k sheets of quads (two triangles each): 2 components"""
    g = np.arange(k + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.column_stack([x.ravel(), y.ravel(), np.zeros(x.size)]).astype(np.float64)
    a = (x[:-1, :-1] * (k + 1) + y[:-1, :-1]).ravel()
    t = np.concatenate([np.column_stack([a, a + k + 1, a + 1]), np.column_stack([a + 1, a + k + 1, a + k + 2])])
    verts = np.concatenate([v * 0.01, v * 0.013 + np.array([0.0, 0.0, 1.0])])
    return verts, np.concatenate([t, t + v.shape[0]]).astype(np.int32)


def operators(pkg, scale):
    """(name, call) in the order of round 1; a call returns its outputs as arrays"""
    geo, reg, chg = pkg.geometry, pkg.pipelines.registration, pkg.change_detection
    pc = lambda seed, n: geo.PointCloud(cloud(seed, n * scale))

    def icp():
        src, tgt = cloud(5, 1200 * scale), cloud(6, 1500 * scale)
        init = np.eye(4)
        init[:3, 3] = (0.01, -0.02, 0.015)
        r = reg.registration_icp(geo.PointCloud(src), geo.PointCloud(tgt), 0.1, init,
                                 criteria=reg.ICPConvergenceCriteria(max_iteration=8))
        return r.transformation, [r.fitness, r.inlier_rmse], np.asarray(r.correspondence_set)

    def normals():
        p = pc(4, 2500)
        p.estimate_normals(geo.KDTreeSearchParamKNN(12))
        return np.asarray(p.normals), np.asarray(p.covariances)

    def voxel():
        return (np.asarray(pc(8, 3000).voxel_down_sample(0.05).points),)

    def plane():
        model, inliers = pc(10, 1300).segment_plane(0.01, 3, 200, seed=3)
        return model, np.asarray(inliers, np.int64)

    def components():
        v, t = sheets(12 * scale)
        labels, counts, areas = geo.TriangleMesh(v, t).cluster_connected_triangles()
        return np.asarray(labels, np.int32), np.asarray(counts, np.int64), np.asarray(areas)

    return [
        ("sor", lambda: (np.asarray(pc(1, 3000).remove_statistical_outlier(20, 2.0)[1], np.int64),)),
        ("ror", lambda: (np.asarray(pc(2, 1700).remove_radius_outlier(6, 0.08)[1], np.int64),)),
        ("dbscan", lambda: (np.asarray(pc(3, 900).cluster_dbscan(0.12, 5), np.int32),)),
        ("normals", normals),
        ("icp", icp),
        ("distance", lambda: (np.asarray(pc(7, 800).compute_point_cloud_distance(pc(17, 2100))),)),
        ("voxel", voxel),
        ("key_diff", lambda: chg.voxel_key_diff(cloud(9, 2000 * scale), cloud(19, 1800 * scale), 0.05, (0, 0, 0))),
        ("plane", plane),
        ("components", components),
    ]


def run_round(pkg, scale, reverse):
    ops = operators(pkg, scale)
    out = {}
    for name, call in (reversed(ops) if reverse else ops):
        out[name] = [np.asarray(a) for a in call()]
    return out


def assert_rounds_equal(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert len(a[name]) == len(b[name])
        for i, (x, y) in enumerate(zip(a[name], b[name])):
            assert_bitwise(x, y, f"{what}: {name}[{i}]")


def child(root, pkg_name, dst):
    import importlib

    sys.path.insert(0, root)
    pkg = importlib.import_module(pkg_name)
    import torch

    torch.cuda.set_device(0)
    out = run_round(pkg, 2, True)
    np.savez(dst, **{f"{name}_{i}": a for name, arrs in out.items() for i, a in enumerate(arrs)})


@pytest.mark.gpu
def test_rounds_agree_across_growth_and_reuse(gpu, pkg, tmp_path):
    lib = __import__("importlib").import_module(PKG + "._lib")
    first = run_round(pkg, 1, False)
    grown = run_round(pkg, 2, True)
    again = run_round(pkg, 1, False)
    print(f"otx_alloc_count after the three rounds: {lib.alloc_count()}")
    for name, arrs in first.items():  # the rounds did find something: no comparison of empty outputs
        assert all(a.size > 0 for a in arrs), name
    assert len(np.unique(first["dbscan"][0])) > 2 and first["components"][1].tolist() == [288, 288]
    assert_rounds_equal(first, again, "round 1 vs round 3")
    dst = tmp_path / "fresh.npz"
    run = subprocess.run([sys.executable, __file__, ROOT, PKG, str(dst)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(dst)
    fresh = {name: [got[f"{name}_{i}"] for i in range(len(arrs))] for name, arrs in grown.items()}
    assert_rounds_equal(grown, fresh, "round 2 vs a fresh process")


if __name__ == "__main__":
    child(*sys.argv[1:4])
