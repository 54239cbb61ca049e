"""Exhaustive numpy statement of pipelines.registration.compute_fpfh_feature and correspondences_from_features
(DESIGN.md §4 "features"): what csrc/features.hip must compute.  Everything is float64 with every operation rounded on
its own, in the order written here; sequential sums are numpy cumulative sums (strictly left to right).

The neighbour list of point i is normals_ref.neighbours' (ascending (d2, index), the first min(k, n), hybrid: of these
the ones with d2 < radius radius); entry 0 is skipped as "the query itself" whatever index it holds.

Only acos and atan2 may differ in their last bits between this file and the device library.  acos decides a swap and
atan2 a bin, so a difference shows only where a comparison is nearly a tie: such points are marked *fragile*
(FRAGILE_EPS) and left out of bit-for-bit comparisons.
"""
import numpy as np

import normals_ref as NR

BINS = 33
FRAGILE_EPS = 1e-9
TWO_PI = 2.0 * np.pi


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(p1, n1, P2, N2):
    """(f [m][3] = (f1, f2, f3) of point (p1, n1) against the m points (P2, N2), close [m]: the two acos values of a
    pair with |a1| != |a2| differ by less than FRAGILE_EPS)"""
    p1, n1 = np.asarray(p1, np.float64), np.asarray(n1, np.float64)
    P2, N2 = np.asarray(P2, np.float64).reshape(-1, 3), np.asarray(N2, np.float64).reshape(-1, 3)
    m = len(P2)
    with np.errstate(all="ignore"):
        dp = P2 - p1
        dist = np.sqrt(_dot(dp, dp))
        a1 = _dot(n1[None, :], dp) / dist
        a2 = _dot(N2, dp) / dist
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = c1 > c2  # a NaN compares false: no swap
        close = (np.abs(a1) != np.abs(a2)) & (np.abs(c1 - c2) < FRAGILE_EPS) & (dist != 0)
        A = np.where(swap[:, None], N2, np.broadcast_to(n1, (m, 3)))
        B = np.where(swap[:, None], np.broadcast_to(n1, (m, 3)), N2)
        dp = np.where(swap[:, None], -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = _cross(dp, A)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(A, v)
        f2 = _dot(v, B)
        f1 = np.arctan2(_dot(w, B), _dot(A, B))
        f = np.stack([f1, f2, f3], axis=-1)
        f[(dist == 0) | (vn == 0)] = 0.0
    return f, close


def bin_coordinates(f):
    """the unclamped bin coordinates [m][3] of pair features [m][3]"""
    f = np.asarray(f, np.float64)
    return np.stack([11 * (f[:, 0] + np.pi) / TWO_PI, 11 * (f[:, 1] + 1.0) * 0.5, 11 * (f[:, 2] + 1.0) * 0.5], axis=-1)


def bins(c):
    """floor, clamped to 0 .. 10 (a NaN lands in bin 0)"""
    with np.errstate(all="ignore"):
        h = np.floor(c)
        h = np.where(h >= 0.0, h, 0.0)
        h = np.where(h > 10.0, 10.0, h)
    return h.astype(np.int64)


def lists(P, k, radius=None):
    """per point (L: the neighbour indices, D2: their squared distances)"""
    P = np.ascontiguousarray(P, np.float64)
    out = []
    for i, L in enumerate(NR.neighbours(P, k, radius)):
        d = P[L] - P[i]
        out.append((L, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return out


def spfh(P, N, nbl):
    """(S [n][33], fragile [n])"""
    P, N = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(N, np.float64)
    n = len(P)
    S = np.zeros((n, BINS))
    fragile = np.zeros(n, bool)
    for i, (L, _) in enumerate(nbl):
        if len(L) <= 1:
            continue
        inc = np.float64(100.0) / np.float64(len(L) - 1)
        f, close = pair_features(P[i], N[i], P[L[1:]], N[L[1:]])
        c = bin_coordinates(f)
        with np.errstate(all="ignore"):
            r = np.rint(c)
            near = (r >= 1) & (r <= 10) & (np.abs(c - r) < FRAGILE_EPS)  # 0 and 11: both sides clamp to one bin
        fragile[i] = bool(near.any() or close.any())
        h = bins(c)
        for t in range(len(h)):  # in list order
            S[i, h[t, 0]] += inc
            S[i, 11 + h[t, 1]] += inc
            S[i, 22 + h[t, 2]] += inc
    return S, fragile


def fpfh_from_spfh(S, nbl, s_fragile=None):
    """(F [n][33], fragile [n]: the point's own SPFH or a list member's is fragile)"""
    n = len(S)
    F = np.zeros((n, BINS))
    fragile = np.zeros(n, bool)
    for i, (L, D2) in enumerate(nbl):
        if s_fragile is not None:
            fragile[i] = bool(s_fragile[i] or s_fragile[L].any())
        if len(L) <= 1:
            continue
        keep = D2[1:] != 0
        Lk, Dk = L[1:][keep], D2[1:][keep]
        acc = np.zeros(BINS)
        total = np.zeros(3)
        if len(Lk):
            val = S[Lk] / Dk[:, None]  # [t][j]
            acc = np.cumsum(val, axis=0)[-1]  # per j, in neighbour order
            for c in range(3):  # neighbour outer, component inner
                total[c] = np.cumsum(val[:, c * 11:(c + 1) * 11].ravel())[-1]
        for c in range(3):
            if total[c] != 0:
                total[c] = np.float64(100.0) / total[c]
        acc = acc * np.repeat(total, 11)
        F[i] = acc + S[i]
    return F, fragile


def compute(P, N, k, radius=None):
    """dict: lists, spfh [n][33], fpfh [n][33], spfh_fragile [n], fpfh_fragile [n]"""
    nbl = lists(P, k, radius)
    S, sf = spfh(P, N, nbl)
    F, ff = fpfh_from_spfh(S, nbl, sf)
    return {"lists": nbl, "spfh": S, "fpfh": F, "spfh_fragile": sf, "fpfh_fragile": ff}


# ------------------------------------------------------------------------------------------------ matching
def nearest(src, tgt):
    """per row of src [n][dim] the row of tgt [m][dim] with the smallest (d2, index); d2 summed over j in order"""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    d2 = np.zeros((len(src), len(tgt)))
    for j in range(src.shape[1]):
        df = src[:, j, None] - tgt[None, :, j]
        d2 += df * df
    return np.argmin(d2, axis=1).astype(np.int32)  # the first minimum: ties to the lowest index


def correspondences(src, tgt, mutual_filter=False, ratio=0.1):
    """(pairs [k][2] int32, fell_back)"""
    n = len(src)
    ms = nearest(src, tgt)
    every = np.stack([np.arange(n, dtype=np.int32), ms], axis=1)
    if not mutual_filter:
        return every, False
    mt = nearest(tgt, src)
    kept = every[mt[ms] == np.arange(n)]
    if float(len(kept)) >= np.float64(ratio) * float(n):
        return kept, False
    return every, True
