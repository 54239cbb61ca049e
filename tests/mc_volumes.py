"""Designed TSDF volumes for the marching-cubes parity tests (tests/test_mc_designed.py on the CPU,
tests/test_gpu_mc_designed.py on the GPU): what a scanned volume -- a smooth thin shell with whole-count weights and
every neighbour unit present across the surface -- never gives.  numpy only.

Every builder returns (keys int32 [U][3] sorted, tsdf f32 [U][4096], weight f32 [U][4096], color f64 [U][4096][3]) in
export_units' layout (voxel order x*256 + y*16 + z, colours 0..255) from a fixed seed.  analyse() restates, on the dense
voxel grid, which cubes Open3D's ExtractTriangleMesh skips, each cube's configuration and the set of cut edges that get
a vertex: the CPU test uses it to check that a case is what it claims to be.
"""
import numpy as np

RES = 16
VOXEL_LENGTH = 0.01
FAR_VOXEL_LENGTHS = (0.005, 0.01, 0.037)
DENORM = np.float32(1.4e-45)  # the smallest float32 denormal

SHIFT = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
E2V = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
ESHIFT = [(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 1, 1), (0, 1, 1, 0),
          (0, 0, 1, 1), (0, 0, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2), (0, 1, 0, 2)]

BLOCK_KEYS = np.array([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)  # sorted
ORIGIN_KEY = (-1, -1, -1)  # the unit of the block whose seven +x/+y/+z neighbours are the block's other units


def split(keys, lo, tsdf, weight, color):
    """the units `keys` cut out of dense arrays whose element [0, 0, 0] is the voxel RES * lo"""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    lo = np.asarray(lo)
    t, w, c = [], [], []
    for k in keys:
        o = (k - lo) * RES
        s = (slice(o[0], o[0] + RES), slice(o[1], o[1] + RES), slice(o[2], o[2] + RES))
        t.append(tsdf[s].reshape(-1))
        w.append(weight[s].reshape(-1))
        c.append(color[s].reshape(-1, 3))
    return (keys, np.stack(t).astype(np.float32), np.stack(w).astype(np.float32), np.stack(c).astype(np.float64))


def _noise_dense(shape, seed):
    rng = np.random.default_rng(seed)
    tsdf = rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)  # uniform in [-1, 1), exact in float32
    weight = np.ones(shape, np.float32)
    color = rng.uniform(0.0, 255.0, shape + (3,))
    return rng, tsdf, weight, color


def noise():
    """2 x 2 x 2 units at keys -1..0, white-noise tsdf, weight 1 everywhere: every cube configuration, about three
    vertices and two and a half triangles per voxel (the emission lists near their worst case)"""
    _, t, w, c = _noise_dense((32, 32, 32), 101)
    return split(BLOCK_KEYS, (-1, -1, -1), t, w, c)


def checkerboard():
    """the same block with the sign of the tsdf by the parity of x + y + z: in the unit ORIGIN_KEY every one of the
    3 * 4096 edges is cut and every cube emits"""
    rng = np.random.default_rng(102)
    mag = np.float32(0.05) + np.float32(0.9) * rng.random((32, 32, 32), dtype=np.float32)
    g = np.indices((32, 32, 32)).sum(0)  # the parity of the dense index is that of the voxel coordinate (offset 16 * 3)
    t = np.where(g & 1, -mag, mag).astype(np.float32)
    w = np.ones((32, 32, 32), np.float32)
    c = rng.uniform(0.0, 255.0, (32, 32, 32, 3))
    return split(BLOCK_KEYS, (-1, -1, -1), t, w, c)


HOLES_FACE_UNIT = (0, -1, 0)  # the unit whose whole x == 0 face has weight 0


def holes():
    """noise with about 30 % of the weights 0 at random, the whole x == 0 face of HOLES_FACE_UNIT at weight 0, and
    voxel (0, 0, 0) of unit (0, 0, 0) at weight 0: skipped cubes whose edges valid cubes next to them still use"""
    rng, t, w, c = _noise_dense((32, 32, 32), 103)
    w[rng.random((32, 32, 32)) < 0.3] = 0.0
    fx, fy, fz = ((np.array(HOLES_FACE_UNIT) + 1) * RES).tolist()
    w[fx, fy:fy + RES, fz:fz + RES] = 0.0
    w[16, 16, 16] = 0.0
    return split(BLOCK_KEYS, (-1, -1, -1), t, w, c)


def subset_keys(mask):
    """the block's unit keys without the non-origin units whose bit (index into BLOCK_KEYS[1:]) is set in mask"""
    keep = [0] + [i for i in range(1, 8) if not (mask >> (i - 1)) & 1]
    return BLOCK_KEYS[keep]


def subsets(mask):
    """noise with a subset (0 <= mask < 128) of the seven non-origin units removed: every present / absent combination
    of the origin unit's + neighbours, and vertices on the low faces of units whose - neighbours are absent"""
    keys, t, w, c = noise()
    keep = [0] + [i for i in range(1, 8) if not (mask >> (i - 1)) & 1]
    return keys[keep], t[keep], w[keep], c[keep]


SPECIAL_KEYS = np.array([(2, -3, 1), (3, -3, 1)], np.int32)


def special():
    """one unit and its +x neighbour with planted values: tsdf +0.0, -0.0, the float32 denormals +-1.4e-45, +-1.0 and
    neighbours of equal magnitude and opposite sign; runs of voxels at exactly +0.0 inside negative ones (their
    vertices land on a voxel centre bit for bit, three to a point: zero-area triangles), one of them across the unit
    border; weights 1.4e-45, 1.0, 255.0 and 1e30 (none is zero: Open3D treats a denormal weight as observed and a
    denormal negative tsdf as negative); colours with exact 0 and 255.  No NaN, no inf."""
    shape = (32, 16, 16)
    rng, t, w, c = _noise_dense(shape, 104)
    w[...] = rng.choice(np.array([DENORM, 1.0, 255.0, 1e30], np.float32), shape)
    pick = rng.integers(0, 24, shape)
    for code, val in enumerate([0.0, -0.0, DENORM, -DENORM, 1.0, -1.0]):
        t[pick == code] = np.float32(val)
    pair = np.argwhere(pick[:-1] == 6)  # x neighbours of equal magnitude and opposite sign, also across the border
    t[pair[:, 0] + 1, pair[:, 1], pair[:, 2]] = -t[pair[:, 0], pair[:, 1], pair[:, 2]]
    pair = np.argwhere(pick[:, :, :-1] == 7)
    t[pair[:, 0], pair[:, 1], pair[:, 2] + 1] = -t[pair[:, 0], pair[:, 1], pair[:, 2]]
    t[4:7, 4:7, 1:14] = np.float32(-0.5)  # a run along z at exactly +0.0 inside a negative sleeve
    t[5, 5, 2:13] = np.float32(0.0)
    t[12:20, 9:12, 9:12] = np.float32(-0.25)  # and one along x across the unit border
    t[13:19, 10, 10] = np.float32(0.0)
    cz = rng.integers(0, 8, shape + (3,))
    c[cz == 0] = 0.0
    c[cz == 1] = 255.0
    return split(SPECIAL_KEYS, SPECIAL_KEYS[0], t, w, c)


FAR_KEYS = np.array([(-4096, 3000, 7), (-4096, 3000, 8)], np.int32)


def far():
    """the noise field in two units far from the origin (a unit and its +z neighbour), for FAR_VOXEL_LENGTHS"""
    _, t, w, c = _noise_dense((16, 16, 32), 105)
    return split(FAR_KEYS, FAR_KEYS[0], t, w, c)


CASES = {"noise": noise, "checkerboard": checkerboard, "holes": holes, "special": special, "far": far}


def analyse(keys, tsdf, weight):
    """On the dense grid of the volume's bounding box (element [0, 0, 0] = voxel RES * lo; absent units and one layer
    past the high faces have weight 0): Open3D's ExtractTriangleMesh per cube (A.4) --
      valid [X][Y][Z] bool: none of the cube's 8 corners has weight == 0 (the others are skipped),
      config [X][Y][Z] int: bit i set when corner i's tsdf < 0 (meaningful where valid),
      used [3][X][Y][Z] bool: the edge (voxel, axis) is cut in some valid cube, i.e. it gets a vertex,
      lo: the lowest unit key per axis."""
    keys = np.asarray(keys).reshape(-1, 3)
    lo = keys.min(0)
    n = (keys.max(0) - lo + 1) * RES + 1
    t = np.zeros(n, np.float32)
    w = np.zeros(n, np.float32)
    for k, tu, wu in zip(keys, tsdf, weight):
        o = (k - lo) * RES
        s = (slice(o[0], o[0] + RES), slice(o[1], o[1] + RES), slice(o[2], o[2] + RES))
        t[s] = np.asarray(tu).reshape(RES, RES, RES)
        w[s] = np.asarray(wu).reshape(RES, RES, RES)
    m = n - 1

    def corner(a, i):
        sx, sy, sz = SHIFT[i]
        return a[sx:sx + m[0], sy:sy + m[1], sz:sz + m[2]]

    valid = np.ones(m, bool)
    config = np.zeros(m, np.int64)
    for i in range(8):
        valid &= corner(w, i) != 0
        config |= (corner(t, i) < 0).astype(np.int64) << i
    used = np.zeros((3,) + tuple(n), bool)
    for e in range(12):
        cut = valid & (((config >> E2V[e][0]) & 1) != ((config >> E2V[e][1]) & 1))
        sx, sy, sz, a = ESHIFT[e]
        used[a, sx:sx + m[0], sy:sy + m[1], sz:sz + m[2]] |= cut
    return valid, config, used[:, :m[0], :m[1], :m[2]], lo  # no edge of the padding layer is ever cut in a valid cube
