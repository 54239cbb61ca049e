"""numpy restatement of the voxel-key set difference, single and multi-object (the checker of test_filter_refs.py
and test_gpu_voxel_diff_edges.py).

A point's cell is floor((p - origin) / voxel_size) per axis, the subtraction and the division each a rounded float64
operation, as int64.  Per object: added = cells of the new cloud absent from the old one, removed = the converse, by
Python set difference.  Output int32, sorted lexicographically by the SIGNED (object, x, y, z).  Nothing here knows
how the library packs keys.
"""
import numpy as np


def cells(xyz, voxel_size, origin):
    """int64 [n][3] lattice cells of a cloud (finite coordinates)"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    o = np.asarray(origin, np.float64).reshape(3)
    return np.floor((p - o) / np.float64(voxel_size)).astype(np.int64)


def _cell_set(xyz, voxel_size, origin):
    return {tuple(r) for r in cells(xyz, voxel_size, origin).tolist()}


def voxel_key_diff(new_xyz, old_xyz, voxel_size, origin):
    """(added, removed): int32 [k][3] each, sorted by signed (x, y, z)"""
    a = _cell_set(new_xyz, voxel_size, origin)
    b = _cell_set(old_xyz, voxel_size, origin)
    added = np.array(sorted(a - b), np.int64).reshape(-1, 3)
    removed = np.array(sorted(b - a), np.int64).reshape(-1, 3)
    return added.astype(np.int32), removed.astype(np.int32)


def voxel_key_diff_multi(new_clouds, old_clouds, voxel_size, origin):
    """(added, removed): int32 [k][4] = (object, x, y, z), sorted by signed (object, x, y, z)"""
    assert len(new_clouds) == len(old_clouds)
    added, removed = [], []
    for j, (n, o) in enumerate(zip(new_clouds, old_clouds)):
        if len(n) == 0 and len(o) == 0:
            continue
        a = _cell_set(n, voxel_size, origin)
        b = _cell_set(o, voxel_size, origin)
        added += [(j,) + c for c in sorted(a - b)]
        removed += [(j,) + c for c in sorted(b - a)]
    return (np.array(added, np.int64).reshape(-1, 4).astype(np.int32),
            np.array(removed, np.int64).reshape(-1, 4).astype(np.int32))
