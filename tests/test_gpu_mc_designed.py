"""GPU parity of marching cubes (mc.hip), the vertex-normal walk and the fused extract_sample_min_z on the designed
volumes of tests/mc_volumes.py, bit for bit against the CPU oracle that imported the same arrays (DESIGN.md §4 A.4,
A.5, A.8).  A scanned volume -- every other mesh test's input -- reaches a handful of the 256 cube configurations,
10-30 surface cubes per unit, whole-count weights and units whose neighbours are present; these volumes reach the
emission lists' worst case, every configuration, skipped cubes beside valid ones, absent neighbour units in every
combination, zeros, denormals and zero-area triangles.  tests/test_mc_designed.py checks (on the CPU) that each volume
is what it claims.  Everything goes through the facade, and so the C ABI; every comparison is assert_bitwise."""
import ctypes as C
import importlib

import numpy as np
import pytest

import mc_volumes as MV
from conftest import assert_bitwise
from test_mc_tables import _tri_table

pytestmark = pytest.mark.gpu

VL = MV.VOXEL_LENGTH


def _import(pkg, units, vl=VL, rgb=True, precision=64, shard=None):
    integ = pkg.pipelines.integration
    keys, tsdf, weight, color = units
    ct = integ.TSDFVolumeColorType.RGB8 if rgb else integ.TSDFVolumeColorType.NoColor
    # a designed volume has at most 8 units (and a sharded one a few halo units): a small initial block pool keeps
    # the creation of the many volumes cheap (the default pool is sized for a scan)
    vol = integ.ScalableTSDFVolume(voxel_length=vl, sdf_trunc=0.04, color_type=ct, color_precision=precision,
                                   max_units=64)
    if shard is not None:
        vol.set_shard(*shard)
    if precision == 32 and rgb:
        color = color.astype(np.float32)
    vol.import_units(keys, tsdf, weight, color if rgb else None)
    return vol


def _oracle(O, units, vl=VL):
    ref = O.TSDF(vl, 0.04, 1, 4)
    ref.import_units(*units)
    return ref.extract_triangle_mesh()


_REF = {}


@pytest.fixture(scope="module")
def ref(O):
    """the oracle's mesh of a named case at VL, computed once: (units, V, VC, T)"""
    def get(case):
        if case not in _REF:
            units = MV.CASES[case]()
            _REF[case] = (units,) + _oracle(O, units)
        return _REF[case]
    return get


def _check_mesh(mesh, V, VC, T, what):
    assert (len(mesh.vertices), len(mesh.triangles)) == (V.shape[0], T.shape[0]), \
        f"{what}: {len(mesh.vertices)} vertices / {len(mesh.triangles)} triangles, the oracle has {V.shape[0]} / {T.shape[0]}"
    assert_bitwise(np.asarray(mesh.triangles), T, what + " triangles")
    assert_bitwise(np.asarray(mesh.vertices), V, what + " vertices")
    if VC is None:
        assert not mesh.has_vertex_colors()
    else:
        assert_bitwise(np.asarray(mesh.vertex_colors), VC, what + " vertex colours")


def _check_variants(pkg, O, units, vl, what, colour_variants=True):
    V, VC, T = _oracle(O, units, vl)
    _check_mesh(_import(pkg, units, vl).extract_triangle_mesh(), V, VC, T, what + ", float64 colours")
    if not colour_variants:
        return
    keys, tsdf, weight, color = units
    c32 = color.astype(np.float32)
    V32, VC32, T32 = _oracle(O, (keys, tsdf, weight, c32.astype(np.float64)), vl)
    _check_mesh(_import(pkg, units, vl, precision=32).extract_triangle_mesh(), V32, VC32, T32,
                what + ", float32 colour state")
    _check_mesh(_import(pkg, units, vl, rgb=False).extract_triangle_mesh(), V, None, T, what + ", NoColor")


@pytest.mark.parametrize("case", ["noise", "checkerboard", "holes", "special"])
def test_designed_volume_bitexact(pkg, O, gpu, case):
    _check_variants(pkg, O, MV.CASES[case](), VL, case)


@pytest.mark.parametrize("vl", MV.FAR_VOXEL_LENGTHS)
def test_far_units_bitexact(pkg, O, gpu, vl):
    _check_variants(pkg, O, MV.far(), vl, f"far, voxel length {vl}")


@pytest.mark.parametrize("first", range(0, 128, 8))
def test_neighbour_subsets_bitexact(pkg, O, gpu, first):
    """the noise block without each subset of the origin unit's seven + neighbours (8 subsets per case)"""
    for mask in range(first, first + 8):
        _check_variants(pkg, O, MV.subsets(mask), VL, f"subset {mask:#04x}", colour_variants=False)


def _dev_mesh(torch, nv, nt):
    return (torch.empty((nv, 3), dtype=torch.float64, device="cuda"),
            torch.empty((nv, 3), dtype=torch.float64, device="cuda"),
            torch.empty((nt, 3), dtype=torch.int32, device="cuda"))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _check_dev(dv, dc, dt, V, VC, T, what):
    assert_bitwise(dt.cpu().numpy(), T, what + " triangles")
    assert_bitwise(dv.cpu().numpy(), V, what + " vertices")
    assert_bitwise(dc.cpu().numpy(), VC, what + " vertex colours")


def _expected_keys(units):
    """the merge keys the oracle's loop implies: a vertex per cut edge of a valid cube in (unit key, voxel, axis)
    order, a triangle per table entry of each valid cube in (unit key, voxel) order"""
    keys = units[0]
    valid, config, used, lo = MV.analyse(*units[:3])
    ntri = np.array([len(r) // 3 for r in _tri_table()])
    vk, tk = [], []
    for k in keys:
        o = (k - lo) * 16
        s = (slice(o[0], o[0] + 16), slice(o[1], o[1] + 16), slice(o[2], o[2] + 16))
        bits = np.flatnonzero(np.moveaxis(used[(slice(None),) + s], 0, -1))  # index (x*256 + y*16 + z) * 3 + axis
        vk.append(np.concatenate([np.tile(k, (len(bits), 1)), bits[:, None]], 1))
        tk.append(np.tile(k, (int(ntri[config[s][valid[s]]].sum()), 1)))
    return np.concatenate(vk).astype(np.int32), np.concatenate(tk).astype(np.int32)


@pytest.mark.parametrize("case", ["noise", "checkerboard", "holes"])
def test_routes_keys_and_normals(pkg, O, gpu, ref, case):
    """The three extraction routes of the C ABI and the forked emission give the oracle's bits; the merge keys are the
    ones the oracle's loop implies; the vertex normals by the marching-cubes walk and by the corner sort equal the
    oracle's."""
    import torch

    L = pkg._lib
    lib = L.load()
    units, V, VC, T = ref(case)
    vol = _import(pkg, units)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nv, nt = C.c_int64(0), C.c_int64(0)
    # one call + fetch
    assert lib.ot_tsdf_extract_triangle_mesh(vol._h, C.byref(nv), C.byref(nt), s) == 0, lib.ot_last_error()
    assert (nv.value, nt.value) == (V.shape[0], T.shape[0])
    dv, dc, dt = _dev_mesh(torch, nv.value, nt.value)
    assert lib.ot_tsdf_fetch_triangle_mesh(vol._h, _p(dv), _p(dc), _p(dt), s) == 0, lib.ot_last_error()
    torch.cuda.synchronize()
    _check_dev(dv, dc, dt, V, VC, T, f"{case}: extract + fetch")
    # count + emit
    nv, nt = C.c_int64(0), C.c_int64(0)
    assert lib.ot_tsdf_extract_triangle_mesh_count(vol._h, C.byref(nv), C.byref(nt), s) == 0, lib.ot_last_error()
    assert (nv.value, nt.value) == (V.shape[0], T.shape[0])
    dv, dc, dt = _dev_mesh(torch, nv.value, nt.value)
    assert lib.ot_tsdf_emit_triangle_mesh(vol._h, _p(dv), _p(dc), _p(dt), s) == 0, lib.ot_last_error()
    torch.cuda.synchronize()
    _check_dev(dv, dc, dt, V, VC, T, f"{case}: count + emit")
    # into a capacity that is too small (nothing past it is written), then emit
    small_v, small_t = V.shape[0] // 2, T.shape[0] // 3
    gv, gc, gt = _dev_mesh(torch, small_v + 64, small_t + 64)
    gv[small_v:], gc[small_v:], gt[small_t:] = -7.0, -7.0, -7
    nv, nt = C.c_int64(0), C.c_int64(0)
    st = lib.ot_tsdf_extract_triangle_mesh_into(vol._h, _p(gv), _p(gc), _p(gt), small_v, small_t, C.byref(nv),
                                                C.byref(nt), s)
    assert st == L.OT_ERR_CAPACITY and (nv.value, nt.value) == (V.shape[0], T.shape[0])
    torch.cuda.synchronize()
    assert bool((gv[small_v:] == -7.0).all()) and bool((gc[small_v:] == -7.0).all()) and bool((gt[small_t:] == -7).all())
    dv, dc, dt = _dev_mesh(torch, nv.value, nt.value)
    assert lib.ot_tsdf_emit_triangle_mesh(vol._h, _p(dv), _p(dc), _p(dt), s) == 0, lib.ot_last_error()
    torch.cuda.synchronize()
    _check_dev(dv, dc, dt, V, VC, T, f"{case}: emit after a capacity miss")
    # the forked emission (two kernels on two streams), by count + emit and by _into with room
    L.call("otx_mc_emit_fork", 1)
    try:
        fv, fc, ft = _dev_mesh(torch, V.shape[0], T.shape[0])
        assert lib.ot_tsdf_extract_triangle_mesh_count(vol._h, C.byref(nv), C.byref(nt), s) == 0
        assert lib.ot_tsdf_emit_triangle_mesh(vol._h, _p(fv), _p(fc), _p(ft), s) == 0, lib.ot_last_error()
        torch.cuda.synchronize()
        _check_dev(fv, fc, ft, V, VC, T, f"{case}: forked emission")
        fv, fc, ft = _dev_mesh(torch, V.shape[0] + 5, T.shape[0] + 5)
        assert lib.ot_tsdf_extract_triangle_mesh_into(vol._h, _p(fv), _p(fc), _p(ft), V.shape[0] + 5, T.shape[0] + 5,
                                                      C.byref(nv), C.byref(nt), s) == 0, lib.ot_last_error()
        torch.cuda.synchronize()
        _check_dev(fv[:nv.value], fc[:nv.value], ft[:nt.value], V, VC, T, f"{case}: forked emission, _into")
    finally:
        L.call("otx_mc_emit_fork", 0)
    # merge keys
    mesh, vk, tk = vol.extract_triangle_mesh(with_keys=True)
    _check_mesh(mesh, V, VC, T, f"{case}: facade")
    vk, tk = vk.cpu().numpy(), tk.cpu().numpy()
    order = (((vk[:, 0].astype(np.int64) * 4 + vk[:, 1]) * 4 + vk[:, 2]) << 16) + vk[:, 3]  # unit keys are -1..0
    assert (np.diff(order) > 0).all(), "vertex keys are not strictly ascending in (unit key, edge bit)"
    voxel, axis = vk[:, 3] // 3, vk[:, 3] % 3
    g = vk[:, :3].astype(np.int64) * 16 + np.stack([voxel >> 8, (voxel >> 4) & 15, voxel & 15], 1)
    centre = VL * 0.5 + VL * g.astype(np.float64)
    upper = VL * 0.5 + VL * (g + 1).astype(np.float64)
    rows = np.arange(len(vk))
    along = V[rows, axis]
    assert ((along >= centre[rows, axis]) & (along < upper[rows, axis])).all(), "a vertex left its key's edge"
    off = np.ones_like(V, bool)
    off[rows, axis] = False
    assert_bitwise(V[off], centre[off], f"{case}: vertex coordinates across the key's axis")
    evk, etk = _expected_keys(units)
    assert_bitwise(vk, evk, f"{case}: vertex keys")
    assert_bitwise(tk, etk, f"{case}: triangle unit keys")
    # vertex normals: the walk and the corner sort on the same arrays
    rN = O.vertex_normals(V, T)
    _check_normals(pkg, vol, mesh, rN, case)


def _check_normals(pkg, vol, mesh, rN, what):
    import torch

    L = pkg._lib
    assert mesh._mc is not None
    nv, nt = len(mesh._v), len(mesh._t)
    Vd, Td = mesh._v.dev(), mesh._t.dev()
    walk = torch.empty((nv, 3), dtype=torch.float64, device="cuda")
    st = L.load().ot_tsdf_mesh_vertex_normals(vol._h, mesh._mc[1], _p(Vd), nv, _p(Td), nt, _p(walk), None)
    assert st == 0, L.load().ot_last_error()
    generic = torch.empty_like(walk)
    L.call("ot_mesh_compute_vertex_normals", _p(Vd), nv, _p(Td), nt, _p(generic), None)
    torch.cuda.synchronize()
    assert_bitwise(generic.cpu().numpy(), rN, f"{what}: vertex normals (corner sort)")
    assert_bitwise(walk.cpu().numpy(), rN, f"{what}: vertex normals (marching-cubes walk)")
    mesh.compute_vertex_normals()
    assert_bitwise(np.asarray(mesh.vertex_normals), rN, f"{what}: facade vertex normals")


def test_special_normals(pkg, O, gpu, ref):
    """zero-area triangles and vertices whose normal sum is exactly zero come out as the oracle's values"""
    units, V, VC, T = ref("special")
    vol = _import(pkg, units)
    mesh = vol.extract_triangle_mesh()
    _check_mesh(mesh, V, VC, T, "special")
    rN = O.vertex_normals(V, T)
    assert (rN == 0).all(1).any()
    _check_normals(pkg, vol, mesh, rN, "special")


def test_sharded_noise_merges_bitexact(pkg, O, gpu, ref):
    """noise over 2 ranks: each rank imports its own units and the other's border rows, extracts its own cubes, and
    the partial meshes merge into the unsharded mesh; on each partial mesh the walk equals the corner sort."""
    import torch

    L = pkg._lib
    D = importlib.import_module(pkg.__name__ + ".distributed")
    units, V, VC, T = ref("noise")
    keys = units[0]
    shards, counts = [], []
    for r in range(2):
        probe = _import(pkg, units, shard=(r, 2))  # a sharded volume exports its own units only
        own = {tuple(k) for k in probe.export_units()[0].cpu().numpy().tolist()}
        sel = [i for i, k in enumerate(keys.tolist()) if tuple(k) in own]
        counts.append(len(sel))
        shards.append(_import(pkg, tuple(a[sel] for a in units), shard=(r, 2)))
    assert sum(counts) == len(keys) and min(counts) > 0, counts
    rows = torch.cat([D.pack_border(*v.export_border()) for v in shards])
    parts = []
    for v in shards:
        v.import_border(*D.unpack_border(rows))
        mesh, vk, tk = v.extract_triangle_mesh(with_keys=True)
        parts.append((mesh._v.dev(), mesh._vc.dev(), mesh._t.dev(), vk, tk))
        nv, nt = len(mesh._v), len(mesh._t)
        assert nv > 1000
        walk = torch.empty((nv, 3), dtype=torch.float64, device="cuda")
        generic = torch.empty_like(walk)
        L.call("ot_tsdf_mesh_vertex_normals", v._h, mesh._mc[1], _p(parts[-1][0]), nv, _p(parts[-1][2]), nt, _p(walk),
               None)
        L.call("ot_mesh_compute_vertex_normals", _p(parts[-1][0]), nv, _p(parts[-1][2]), nt, _p(generic), None)
        torch.cuda.synchronize()
        part_V, part_T = parts[-1][0].cpu().numpy(), parts[-1][2].cpu().numpy()
        assert_bitwise(generic.cpu().numpy(), O.vertex_normals(part_V, part_T), "partial mesh normals (corner sort)")
        assert_bitwise(walk.cpu().numpy(), generic.cpu().numpy(), "partial mesh normals (walk vs corner sort)")
    mV, mVC, mT = D.merge_shard_meshes(parts)
    assert sum(p[2].shape[0] for p in parts) == T.shape[0]
    assert_bitwise(mT.cpu().numpy(), T, "merged triangles")
    assert_bitwise(mV.cpu().numpy(), V, "merged vertices")
    assert_bitwise(mVC.cpu().numpy(), VC, "merged vertex colours")


@pytest.mark.parametrize("z_min", [-np.inf, 0.0])
@pytest.mark.parametrize("n_points", [1, 257, 1000])
def test_fused_extract_sample_min_z_on_noise(pkg, O, gpu, ref, n_points, z_min):
    """~10^5 triangles against 1..1000 points: every 256-point tile spans far more triangles than the counts the fused
    sampler stages.  The volume's first extraction takes the separate calls, the second the fused C entry."""
    units, V, VC, T = ref("noise")
    assert T.shape[0] > 8 * 8192
    P, _, PC = O.sample_points_uniformly(V, T, n_points, 11, VC=VC)
    rx, rc = O.filter_min_z(P, PC, z_min)
    rN = O.vertex_normals(V, T)
    vol = _import(pkg, units)
    for tag in ("separate calls", "fused C entry"):
        mesh, cloud = vol.extract_mesh_and_sample_min_z(n_points, z_min, seed=11)
        _check_mesh(mesh, V, VC, T, f"noise, {tag}")
        assert_bitwise(np.asarray(cloud.points), rx, f"cloud points ({tag})")
        assert_bitwise(np.asarray(cloud.colors), rc, f"cloud colours ({tag})")
        assert_bitwise(np.asarray(mesh.vertex_normals), rN, f"vertex normals ({tag})")
        assert getattr(vol, "_mesh_cap", (0, 0))[0] >= V.shape[0]
    if z_min == -np.inf:
        assert len(rx) == n_points
