"""The designed volumes of tests/mc_volumes.py are what they claim to be -- checked on the CPU, on the oracle and on
mc_volumes.analyse (a dense numpy restatement of which cubes Open3D's ExtractTriangleMesh skips, their configurations
and the cut edges that get a vertex).  These are conditions on the test inputs, not measurements of the kernels:
tests/test_gpu_mc_designed.py compares the GPU with the oracle on the same volumes."""
import numpy as np
import pytest

import mc_volumes as MV
from test_mc_tables import _tri_table


def _ntri():
    return np.array([len(r) // 3 for r in _tri_table()])


def _oracle_mesh(O, units, vl=MV.VOXEL_LENGTH):
    vol = O.TSDF(vl, 0.04, 1, 4)
    vol.import_units(*units)
    return vol.extract_triangle_mesh()


def _emitting(valid, config):
    return valid & (config != 0) & (config != 255)


@pytest.mark.parametrize("case", sorted(MV.CASES))
def test_analyse_counts_match_the_oracle(O, case):
    """the dense restatement and the oracle's loop agree on the number of vertices and triangles of every case"""
    units = MV.CASES[case]()
    V, VC, T = _oracle_mesh(O, units)
    valid, config, used, _ = MV.analyse(*units[:3])
    assert V.shape[0] == int(used.sum()) > 0
    assert T.shape[0] == int(_ntri()[config[valid]].sum()) > 0
    assert np.isfinite(V).all() and np.isfinite(VC).all()
    assert T.min() == 0 and T.max() == V.shape[0] - 1


def test_noise_has_every_configuration():
    keys, tsdf, weight, _ = MV.noise()
    assert keys.tolist() == MV.BLOCK_KEYS.tolist() and (weight == 1).all()
    assert tsdf.dtype == np.float32 and tsdf.min() >= -1 and tsdf.max() < 1
    valid, config, used, lo = MV.analyse(keys, tsdf, weight)
    assert lo.tolist() == [-1, -1, -1] and int(valid.sum()) == 31 ** 3
    hist = np.bincount(config[valid], minlength=256)
    assert (hist[1:255] > 0).all(), f"configurations absent from noise: {np.nonzero(hist[1:255] == 0)[0] + 1}"
    # cubes of one unit whose cut edges belong to the +x / +y / +z neighbour units (their vertices are another unit's)
    emit = _emitting(valid, config)
    assert emit[15].any() and emit[:, 15].any() and emit[:, :, 15].any() and emit[15, 15, 15]
    # far more than the counts staged per tile by the fused sampler
    assert int(_ntri()[config[valid]].sum()) > 8 * 8192


def test_checkerboard_saturates_the_origin_unit():
    keys, tsdf, weight, _ = MV.checkerboard()
    valid, config, used, lo = MV.analyse(keys, tsdf, weight)
    assert tuple(keys[0]) == MV.ORIGIN_KEY == tuple(lo)
    own = (slice(0, 16),) * 3  # the dense range of the unit ORIGIN_KEY
    assert valid[own].all()
    assert int(used[(slice(None),) + own].sum()) == 3 * 4096 == 12288
    confs = np.unique(config[own])
    assert confs.tolist() == [0x5A, 0xA5]
    ntri = _ntri()
    assert ntri[0x5A] == ntri[0xA5]
    assert int(ntri[config[own]].sum()) == 4096 * ntri[0x5A] == 16384


def test_holes_has_used_edges_of_skipped_cubes():
    keys, tsdf, weight, _ = MV.holes()
    frac = float((weight == 0).mean())
    assert 0.25 < frac < 0.4
    at = [tuple(k) for k in keys.tolist()]
    face = weight[at.index(MV.HOLES_FACE_UNIT)].reshape(16, 16, 16)
    assert (face[0] == 0).all()
    assert weight[at.index((0, 0, 0))][0] == 0
    valid, config, used, _ = MV.analyse(keys, tsdf, weight)
    assert _emitting(valid, config).sum() > 500
    orphan = used & ~valid[None]  # an edge with a vertex whose owner voxel's own cube is skipped
    assert orphan.sum() > 100
    fx, fy, fz = ((np.array(MV.HOLES_FACE_UNIT) + 1) * 16).tolist()
    assert not used[:, fx, fy:fy + 16, fz:fz + 16].any()  # no vertex on the dead face ...
    assert used[:, fx + 1, fy:fy + 16, fz:fz + 16].any() and used[:, fx - 1, fy:fy + 16, fz:fz + 16].any()  # but beside it


def test_special_has_zero_area_triangles_and_vertices_on_voxel_centres(O):
    units = MV.special()
    keys, tsdf, weight, color = units
    bits = tsdf.view(np.uint32)
    for planted in (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000):
        assert (bits == planted).any(), hex(planted)
    assert set(np.unique(weight).tolist()) == {float(MV.DENORM), 1.0, 255.0, float(np.float32(1e30))}
    assert np.isfinite(tsdf).all() and (color == 0).any() and (color == 255).any()
    assert color.min() == 0 and color.max() == 255
    vl = MV.VOXEL_LENGTH
    V, VC, T = _oracle_mesh(O, units)
    e1, e2 = V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]
    assert int((np.cross(e1, e2) == 0).all(1).sum()) >= 10, "no zero-area triangle"
    g = np.rint((V - vl * 0.5) / vl)
    on_centre = (vl * 0.5 + vl * g == V).all(1)  # the oracle's own expression for a voxel centre, bit for bit
    assert int(on_centre.sum()) >= 10
    # a denormal weight is an observed voxel and a denormal negative tsdf is negative (Open3D on the CPU)
    valid, config, used, _ = MV.analyse(keys, tsdf, weight)
    assert valid[:-1, :-1, :-1].all()
    assert V.shape[0] == int(used.sum())
    N = O.vertex_normals(V, T)
    assert (N == 0).all(1).any(), "no vertex whose triangles are all degenerate"


def test_far_units():
    keys, tsdf, weight, _ = MV.far()
    assert keys.tolist() == [[-4096, 3000, 7], [-4096, 3000, 8]]
    valid, config, used, _ = MV.analyse(keys, tsdf, weight)
    assert _emitting(valid, config)[:, :, 15].any()  # cubes across the unit border


def test_every_subset_has_vertices_on_a_unit_face():
    """Every volume with more than one unit has vertices whose owner voxel lies in the low face layer of its unit
    (local coordinate 0 along an axis other than the edge's) where the unit's - neighbour along that axis is absent:
    of the four cubes sharing such an edge, two lie in a unit that does not exist.  Where a unit and its + neighbour
    are both present, cubes of the first own cut edges of the second."""
    seen = set()
    full = MV.noise()
    for mask in range(128):
        keys = MV.subset_keys(mask)
        units = MV.subsets(mask)
        assert units[0].tolist() == keys.tolist()
        seen.add(tuple(map(tuple, keys.tolist())))
        if len(keys) == 1:
            continue
        valid, config, used, lo = MV.analyse(*units[:3])
        present = {tuple(k) for k in keys.tolist()}
        found = crossing = 0
        for k in present:
            o = (np.array(k) - lo) * 16
            for b in range(3):
                nb = list(k)
                nb[b] -= 1
                s = [slice(o[0], o[0] + 16), slice(o[1], o[1] + 16), slice(o[2], o[2] + 16)]
                s[b] = o[b]
                layer = used[(slice(None),) + tuple(s)]
                others = [a for a in range(3) if a != b]
                if tuple(nb) not in present:
                    found += int(layer[others].sum())
                else:  # cut edges of this unit's low layer in valid cubes of the - neighbour
                    s[b] = o[b] - 1
                    crossing += int((layer[others] & valid[tuple(s)][None]).sum())
        assert found > 0, f"mask {mask}: no vertex on a face without a - neighbour"
        adjacent = any(tuple(np.array(k) + e) in present for k in present for e in np.eye(3, dtype=int))
        assert (crossing > 0) == adjacent, f"mask {mask}"
    assert len(seen) == 128
    assert MV.subsets(0)[1].tobytes() == full[1].tobytes()
