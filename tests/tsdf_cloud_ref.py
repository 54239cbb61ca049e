"""numpy restatement of ScalableTSDFVolume::ExtractPointCloud / ::ExtractVoxelPointCloud.

Works on export_units()-shaped arrays (keys (U,3) int32, tsdf / weight (U,4096) float32, colour (U,4096,3) float32 or
float64 or None, voxels in Open3D's IndexOf order x*256 + y*16 + z) and emits in the canonical order: units by key,
voxel index, axis.  float32 where A.9 says float32 (numpy float32 arrays: every product, sum and quotient rounds to
float32), float64 elsewhere; numpy's element-wise loops never contract a multiply and an add.
"""
from __future__ import annotations

import numpy as np

RES = 16
_BIAS = 1 << 20
F32 = np.float32
SHIFT = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)


def usable(tsdf, weight):
    return (weight != F32(0.0)) & (tsdf < F32(0.98)) & (tsdf >= F32(-0.98))


def _codes(keys):
    k = np.asarray(keys, np.int64) + _BIAS
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


class _Units:
    """the units in key order and a key -> row lookup (-1: missing)"""

    def __init__(self, keys, tsdf, weight, color):
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        self.keys = keys[order]
        self.codes = _codes(self.keys)  # ascending: the packed key orders as (x, y, z)
        n = len(order)
        self.f = np.ascontiguousarray(np.asarray(tsdf, F32)[order]).reshape(n, RES, RES, RES)
        self.w = np.ascontiguousarray(np.asarray(weight, F32)[order]).reshape(n, RES, RES, RES)
        # (float)color_: a float64 colour narrows to float32 first, a float32 one is used as it is
        self.c = None if color is None else np.asarray(color)[order].astype(F32).reshape(n, RES, RES, RES, 3)

    def find(self, keys):
        keys = np.asarray(keys, np.int64)
        ok = np.all((keys >= -_BIAS) & (keys < _BIAS), axis=-1)
        code = _codes(np.where(ok[..., None], keys, 0))
        if len(self.codes) == 0:
            return np.full(code.shape, -1, np.int64)
        pos = np.minimum(np.searchsorted(self.codes, code), len(self.codes) - 1)
        return np.where(ok & (self.codes[pos] == code), pos, -1)


def _centres(keys, idx, vl):
    """(half + vl * index) + (double)key * UL per axis"""
    half, ul = vl * 0.5, vl * float(RES)
    return (half + vl * idx.astype(np.float64)) + keys.astype(np.float64) * ul


def extract_voxel_point_cloud(keys, tsdf, weight, voxel_length):
    """A.10: (points (N,3) f64, colours (N,3) f64)"""
    vl = float(voxel_length)
    un = _Units(keys, tsdf, weight, None)
    u, x, y, z = np.nonzero(usable(un.f, un.w))  # row-major: unit, x, y, z = unit, voxel index
    pts = _centres(un.keys[u], np.stack([x, y, z], 1), vl)
    c = (un.f[u, x, y, z].astype(np.float64) + 1.0) * 0.5
    return pts, np.repeat(c[:, None], 3, 1)


def tsdf_at(un, q, vl, stats=None):
    """GetTSDFAt for q (M,3) f64 -> (M,) f64"""
    ul = vl * float(RES)
    ql = q - 0.5 * vl
    uf = np.floor(ql / ul)
    g = (ql - uf * ul) / vl
    fl = np.floor(g).astype(np.int64)
    i = np.clip(fl, 0, RES - 1)
    r = g - i.astype(np.float64)
    u = uf.astype(np.int64)
    base = un.find(u)
    f = np.zeros((8, len(q)), np.float64)
    for c in range(8):
        cc = i + SHIFT[c]
        uid = un.find(u + (cc >> 4))
        lc = cc & 15
        f[c] = np.where(uid >= 0, un.f[np.maximum(uid, 0), lc[:, 0], lc[:, 1], lc[:, 2]].astype(np.float64), 0.0)
        if stats is not None:
            live = base >= 0
            stats["missing_corners"] += int(np.sum(live & (uid < 0)))
            stats["wrapped_corners"] += int(np.sum(live & np.any(cc >> 4 != 0, axis=1)))
    if stats is not None:
        stats["missing_samples"] += int(np.sum(base < 0))
        stats["clamped"] += int(np.sum(np.any(fl != i, axis=1)))
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    val = (1 - r0) * ((1 - r1) * ((1 - r2) * f[0] + r2 * f[4]) + r1 * ((1 - r2) * f[3] + r2 * f[7])) + \
        r0 * ((1 - r1) * ((1 - r2) * f[1] + r2 * f[5]) + r1 * ((1 - r2) * f[2] + r2 * f[6]))
    return np.where(base >= 0, val, 0.0)


def normal_at(un, p, vl, stats=None):
    """GetNormalAt for p (M,3) f64 -> (M,3) f64"""
    gap = 0.99 * vl
    n = np.zeros_like(p)
    for b in range(3):
        qp, qm = p.copy(), p.copy()
        qp[:, b] = p[:, b] + gap
        qm[:, b] = p[:, b] - gap
        n[:, b] = tsdf_at(un, qp, vl, stats) - tsdf_at(un, qm, vl, stats)
    s = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    pos = s > 0
    n[pos] = n[pos] / np.sqrt(s[pos])[:, None]
    return n


def extract_point_cloud(keys, tsdf, weight, color, voxel_length, normals_at=None, stats=None):
    """A.9.  Returns a dict: points (N,3) f64, colors (N,3) f64 or None (color None: a NoColor volume), normals (M,3)
    f64 of the points normals_at (an index array; None: all of them), edge (N,5) int64 rows (unit key x, y, z, voxel
    index, axis) naming each point's edge.  stats (a dict) receives counts of the paths taken."""
    vl = float(voxel_length)
    un = _Units(keys, tsdf, weight, color)
    n = len(un.keys)
    us = usable(un.f, un.w)
    if stats is not None:
        stats.update(edges_leaving=0, edges_into_missing=0, missing_samples=0, missing_corners=0, wrapped_corners=0,
                     clamped=0)
    emit = np.zeros((n, RES, RES, RES, 3), bool)
    nbs = np.zeros((3, n), np.int64)
    for a in range(3):
        # the neighbour (x, y, z) + e_a: inside the unit, or index 0 of unit k + e_a (missing: w1 = f1 = 0)
        nb = nbs[a] = un.find(un.keys + np.eye(3, dtype=np.int64)[a])
        have = (nb >= 0).reshape((n, 1, 1, 1))
        src = np.maximum(nb, 0)
        f1 = np.concatenate([np.delete(un.f, 0, axis=1 + a),
                             np.where(have, np.take(un.f, [0], axis=1 + a)[src], F32(0))], axis=1 + a)
        w1 = np.concatenate([np.delete(un.w, 0, axis=1 + a),
                             np.where(have, np.take(un.w, [0], axis=1 + a)[src], F32(0))], axis=1 + a)
        emit[..., a] = us & usable(f1, w1) & ((un.f * f1) < F32(0.0))  # a float32 product
        if stats is not None:
            last = np.take(us, [RES - 1], axis=1 + a)
            stats["edges_leaving"] += int(last.sum())
            stats["edges_into_missing"] += int((last & ~have).sum())
    u, x, y, z, a = np.nonzero(emit)  # row-major: unit, voxel index, axis -- the canonical order
    m = len(u)
    rows = np.arange(m)
    idx = np.stack([x, y, z], 1)
    idx1 = idx.copy()
    idx1[rows, a] += 1
    u1 = np.where(idx1[rows, a] == RES, nbs[a, u], u)  # an emitted edge's neighbour is usable, so its unit exists
    idx1 &= RES - 1
    f0 = un.f[u, x, y, z]
    f1 = un.f[u1, idx1[:, 0], idx1[:, 1], idx1[:, 2]]
    r0, r1 = np.abs(f0), np.abs(f1)
    rs = r0 + r1  # float32 sum
    p = _centres(un.keys[u], idx, vl)
    p0a = p[rows, a]
    p1a = p0a + vl
    p[rows, a] = (p0a * r1.astype(np.float64) + p1a * r0.astype(np.float64)) / rs.astype(np.float64)
    colors = None
    if un.c is not None:
        c0 = un.c[u, x, y, z]
        c1 = un.c[u1, idx1[:, 0], idx1[:, 1], idx1[:, 2]]
        colors = (((c0 * r1[:, None] + c1 * r0[:, None]) / rs[:, None]) / F32(255.0)).astype(np.float64)
    sel = rows if normals_at is None else np.asarray(normals_at, np.int64)
    normals = normal_at(un, p[sel], vl, stats)
    edge = np.concatenate([un.keys[u], (x * 256 + y * 16 + z)[:, None], a[:, None]], axis=1)
    return {"points": p, "colors": colors, "normals": normals, "edge": edge}


# ------------------------------------------------------------------------------------------------ fixtures
SPHERE_VL, SPHERE_TRUNC, SPHERE_R = 0.01, 0.04, 0.105
SPHERE_CENTRE = (0.004, -0.003, 0.002)


def sphere_units(shift=(0, 0, 0)):
    """The hand-made sphere volume: units {-1, 0}^3 without (0, -1, 0), voxel_length 0.01, sdf_trunc 0.04, RGB8.
    Returns (keys int32 (7,3), tsdf f32 (7,4096), weight f32 (7,4096), colour f64 (7,4096,3)); `shift` moves the
    unit keys only (the voxel values stay those of the unshifted sphere)."""
    keys = np.array([(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0) if (i, j, k) != (0, -1, 0)], np.int64)
    i = np.arange(RES)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    tsdf = np.zeros((len(keys), RES, RES, RES), F32)
    weight = np.zeros_like(tsdf)
    color = np.zeros((len(keys), RES, RES, RES, 3), np.float64)
    rgb = np.stack([(16 * x + y) % 256, (16 * y + z) % 256, (16 * z + x) % 256], -1).astype(np.float64)
    for n, k in enumerate(keys):
        d = [(0.005 + 0.01 * g) + float(k[ax]) * 0.16 - SPHERE_CENTRE[ax] for ax, g in enumerate((x, y, z))]
        sdf = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - SPHERE_R
        obs = sdf > -SPHERE_TRUNC
        tsdf[n] = np.where(obs, np.minimum(1.0, sdf / SPHERE_TRUNC).astype(F32), F32(0))
        weight[n] = np.where(obs, F32(1), F32(0))
        color[n] = np.where(obs[..., None], rgb, 0.0)
    keys = (keys + np.asarray(shift, np.int64)).astype(np.int32)
    return keys, tsdf.reshape(-1, 4096), weight.reshape(-1, 4096), color.reshape(-1, 4096, 3)


SLAB_VL = 1.0 / 64.0
SLAB_LOW, SLAB_HIGH = 3.25, 11.75  # the two faces, in voxel indices along z


def slab_units():
    """A slab between two planes z = const, four units {-1, 0}^2 x {0}, voxel_length 2^-6, every voxel observed:
    tsdf(z) = (|z - 7.5| - 4.25) / 4, all dyadic, so every operation of A.9 is exact -- the points sit at voxel index
    3.25 and 11.75 along z and the tsdf interpolated there is exactly 0."""
    keys = np.array([(i, j, 0) for i in (-1, 0) for j in (-1, 0)], np.int32)
    z = np.arange(RES, dtype=np.float64)
    col = ((np.abs(z - 7.5) - 4.25) / 4.0).astype(F32)
    tsdf = np.broadcast_to(col, (len(keys), RES, RES, RES)).reshape(len(keys), 4096).copy()
    return keys, tsdf, np.ones_like(tsdf), None


def dense_units():
    """Two units (0, 0, 0) and (1, 0, 0) whose tsdf alternates in sign from voxel to voxel with varying magnitude, so
    nearly every edge is cut: thousands of points per unit (a scan's unit holds a few hundred), with a few unobserved
    voxels and a few beyond +-0.98.  RGB8, voxel_length 0.01."""
    keys = np.array([(0, 0, 0), (1, 0, 0)], np.int32)
    i = np.arange(RES)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    tsdf = np.zeros((2, RES, RES, RES), F32)
    weight = np.ones_like(tsdf)
    color = np.zeros((2, RES, RES, RES, 3), np.float64)
    for n in range(2):
        sign = np.where((x + y + z + n) % 2 == 0, 1.0, -1.0)
        mag = 0.1 + 0.07 * ((x * 7 + y * 3 + z * 5 + n) % 13)  # up to 0.94; every 29th voxel pushed beyond 0.98
        mag = np.where((x * 256 + y * 16 + z) % 29 == 7, 0.99, mag)
        tsdf[n] = (sign * mag).astype(F32)
        weight[n] = np.where((x * 256 + y * 16 + z) % 31 == 5, F32(0), F32(2))
        tsdf[n] = np.where(weight[n] == 0, F32(0), tsdf[n])
        color[n] = np.stack([(x * 16 + n) % 256, (y * 16 + z) % 256, (z * 13 + x * 5) % 256], -1) + 0.25
    return keys, tsdf.reshape(-1, 4096), weight.reshape(-1, 4096), color.reshape(-1, 4096, 3)
