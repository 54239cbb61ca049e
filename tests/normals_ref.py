"""Exhaustive O(n^2) numpy statement of PointCloud.estimate_covariances / estimate_normals and the orientation calls
(DESIGN.md §4 "normals"): what csrc/normals.hip must compute.  Everything is float64 with every operation rounded on
its own, in the order written here; the solver can also run in np.longdouble, which measures how sensitive a point's
normal is to rounding (the tolerance of tests/test_gpu_normals.py).

Neighbours of point i: all points j (i included) ascending by (d2, j), d2 = ((dx dx) + dy dy) + dz dz; the first
min(k, n); hybrid search keeps of these the ones with d2 < radius radius.  Covariance: identity below 3 neighbours,
else nine sequential sums in neighbour order, divided by the count, C = E[pp^T] - E[p]E[p]^T without centring.
Normal: Open3D's FastEigen3x3 (Eberly's non-iterative symmetric 3x3 solver).
"""
import numpy as np

PATH_FEW, PATH_ZERO, PATH_DIAGONAL, PATH_TRIG = 0, 1, 2, 3
TWO_THIRDS_PI = 2.09439510239319549


# ------------------------------------------------------------------------------------------------ neighbours
def neighbours(P, k, radius=None):
    """per point the neighbour indices in (d2, index) order"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    idx = np.arange(n)
    out = []
    for i in range(n):
        d = P - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((idx, d2))[:min(k, n)]  # last key first: d2, ties by index
        if radius is not None:
            order = order[d2[order] < np.float64(radius) * np.float64(radius)]
        out.append(order)
    return out


def covariance(P, nb):
    if len(nb) < 3:
        return np.eye(3)
    s = np.zeros(9)
    for j in nb:  # sequential: the order is part of the result
        x, y, z = P[j]
        s[0] += x
        s[1] += y
        s[2] += z
        s[3] += x * x
        s[4] += x * y
        s[5] += x * z
        s[6] += y * y
        s[7] += y * z
        s[8] += z * z
    s = s / np.float64(len(nb))
    C = np.empty((3, 3))
    C[0, 0] = s[3] - s[0] * s[0]
    C[1, 1] = s[6] - s[1] * s[1]
    C[2, 2] = s[8] - s[2] * s[2]
    C[0, 1] = C[1, 0] = s[4] - s[0] * s[1]
    C[0, 2] = C[2, 0] = s[5] - s[0] * s[2]
    C[1, 2] = C[2, 1] = s[7] - s[1] * s[2]
    return C


# ------------------------------------------------------------------------------------------------ the solver
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _eigvec0(A, e):
    """the longest cross product of two rows of A - e I (the first wins ties), normalised"""
    r0 = (A[0][0] - e, A[0][1], A[0][2])
    r1 = (A[0][1], A[1][1] - e, A[1][2])
    r2 = (A[0][2], A[1][2], A[2][2] - e)
    c = (_cross(r0, r1), _cross(r0, r2), _cross(r1, r2))
    d = [_dot(v, v) for v in c]
    im, dm = 0, d[0]
    if d[1] > dm:
        im, dm = 1, d[1]
    if d[2] > dm:
        im, dm = 2, d[2]
    s = np.sqrt(dm)
    return tuple(x / s for x in c[im])


def _eigvec1(A, v, e1, one):
    if abs(v[0]) > abs(v[1]):
        inv = one / np.sqrt(v[0] * v[0] + v[2] * v[2])
        U = (-v[2] * inv, one * 0, v[0] * inv)
    else:
        inv = one / np.sqrt(v[1] * v[1] + v[2] * v[2])
        U = (one * 0, v[2] * inv, -v[1] * inv)
    W = _cross(v, U)
    AU = tuple(_dot(A[i], U) for i in range(3))
    AW = tuple(_dot(A[i], W) for i in range(3))
    m00, m01, m11 = _dot(U, AU) - e1, _dot(U, AW), _dot(W, AW) - e1
    a00, a01, a11 = abs(m00), abs(m01), abs(m11)
    if a00 >= a11:
        if not max(a00, a01) > 0:
            return U
        if a00 >= a01:
            m01 = m01 / m00
            m00 = one / np.sqrt(one + m01 * m01)
            m01 = m01 * m00
        else:
            m00 = m00 / m01
            m01 = one / np.sqrt(one + m00 * m00)
            m00 = m00 * m01
        return tuple(m01 * U[i] - m00 * W[i] for i in range(3))
    if not max(a11, a01) > 0:
        return U
    if a11 >= a01:
        m01 = m01 / m11
        m11 = one / np.sqrt(one + m01 * m01)
        m01 = m01 * m11
    else:
        m11 = m11 / m01
        m01 = one / np.sqrt(one + m11 * m11)
        m11 = m11 * m01
    return tuple(m11 * U[i] - m01 * W[i] for i in range(3))


def fast_eigen(C, F=np.float64):
    """(eigenvector of the smallest eigenvalue as a float64 [3], path code 1..3) of the symmetric float64 C, every
    operation in F"""
    with np.errstate(all="ignore"):
        Cf = [[F(C[i, j]) for j in range(3)] for i in range(3)]
        mx = max(max(row) for row in Cf)
        if mx == 0:
            return np.zeros(3), PATH_ZERO
        A = [[Cf[i][j] / mx for j in range(3)] for i in range(3)]
        norm = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2]
        if not norm > 0:
            if A[0][0] < A[1][1] and A[0][0] < A[2][2]:
                return np.array([1.0, 0.0, 0.0]), PATH_DIAGONAL
            if A[1][1] < A[0][0] and A[1][1] < A[2][2]:
                return np.array([0.0, 1.0, 0.0]), PATH_DIAGONAL
            return np.array([0.0, 0.0, 1.0]), PATH_DIAGONAL
        one = F(1)
        q = ((A[0][0] + A[1][1]) + A[2][2]) / F(3)
        b00, b11, b22 = A[0][0] - q, A[1][1] - q, A[2][2] - q
        p = np.sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + norm * F(2)) / F(6))
        c00 = b11 * b22 - A[1][2] * A[1][2]
        c01 = A[0][1] * b22 - A[1][2] * A[0][2]
        c02 = A[0][1] * A[1][2] - b11 * A[0][2]
        det = ((b00 * c00 - A[0][1] * c01) + A[0][2] * c02) / ((p * p) * p)
        h = det * F(0.5)
        if h < -1:
            h = F(-1)
        if h > 1:
            h = F(1)
        ang = np.arccos(h) / F(3)
        beta2 = np.cos(ang) * F(2)
        beta0 = np.cos(ang + F(TWO_THIRDS_PI)) * F(2)
        beta1 = -(beta0 + beta2)
        e0, e1, e2 = q + p * beta0, q + p * beta1, q + p * beta2
        if h >= 0:
            v2 = _eigvec0(A, e2)
            if e2 < e0 and e2 < e1:
                v = v2
            else:
                v1 = _eigvec1(A, v2, e1, one)
                v = v1 if (e1 < e0 and e1 < e2) else _cross(v1, v2)
        else:
            v0 = _eigvec0(A, e0)
            if e0 < e1 and e0 < e2:
                v = v0
            else:
                v1 = _eigvec1(A, v0, e1, one)
                v = v1 if (e1 < e0 and e1 < e2) else _cross(v0, v1)
        return np.array([float(x) for x in v], np.float64), PATH_TRIG


def _finish(v, old):
    """estimate_normals' last step: a zero result takes the prior (or +z), a prior orients the result"""
    v = np.array(v, np.float64)
    if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] == 0:
        v = np.array([0.0, 0.0, 1.0]) if old is None else np.array(old, np.float64)
    if old is not None and (v[0] * old[0] + v[1] * old[1]) + v[2] * old[2] < 0:
        v = -v
    return v


def estimate(P, k, radius=None, prior=None, longdouble=False):
    """dict: nbrs (list of index arrays), cov [n][3][3], normals [n][3], path [n], gap [n] = (w1 - w0) / w2 of
    numpy.linalg.eigh (0 where w2 <= 0), and with longdouble=True normals_ld: the solver run in np.longdouble on the
    same float64 covariances"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    nbrs = neighbours(P, k, radius)
    cov = np.zeros((n, 3, 3))
    nrm = np.zeros((n, 3))
    nld = np.zeros((n, 3))
    path = np.zeros(n, np.int32)
    gap = np.zeros(n)
    for i in range(n):
        cov[i] = covariance(P, nbrs[i])
        v, pc = fast_eigen(cov[i])
        path[i] = PATH_FEW if len(nbrs[i]) < 3 else pc
        old = None if prior is None else prior[i]
        nrm[i] = _finish(v, old)
        w = np.linalg.eigh(cov[i])[0]
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        if longdouble:
            nld[i] = _finish(fast_eigen(cov[i], np.longdouble)[0], old)
    out = {"nbrs": nbrs, "cov": cov, "normals": nrm, "path": path, "gap": gap}
    if longdouble:
        out["normals_ld"] = nld
    return out


# ------------------------------------------------------------------------------------------------ orientation
def _sq(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def orient_to_direction(N, ref):
    N = np.array(N, np.float64)
    ref = np.asarray(ref, np.float64)
    for i in range(len(N)):
        if _sq(N[i]) == 0:
            N[i] = ref
        elif (N[i, 0] * ref[0] + N[i, 1] * ref[1]) + N[i, 2] * ref[2] < 0:
            N[i] = -N[i]
    return N


def orient_to_camera(N, P, cam):
    N = np.array(N, np.float64)
    cam = np.asarray(cam, np.float64)
    for i in range(len(N)):
        v = cam - P[i]
        if _sq(N[i]) == 0:
            s = _sq(v)
            N[i] = np.array([0.0, 0.0, 1.0]) if s == 0 else v / np.sqrt(s)
        elif (N[i, 0] * v[0] + N[i, 1] * v[1]) + N[i, 2] * v[2] < 0:
            N[i] = -N[i]
    return N


def normalize(N):
    N = np.array(N, np.float64)
    for i in range(len(N)):
        s = _sq(N[i])
        if s > 0:
            N[i] = N[i] / np.sqrt(s)
    return N


def angle(a, b):
    """the angle between the lines of a and b (sign-free), atan2(|a x b|, |a . b|) in long double"""
    a = np.asarray(a, np.longdouble)
    b = np.asarray(b, np.longdouble)
    c = np.cross(a, b)
    s = np.sqrt((c * c).sum(axis=-1))
    d = np.abs((a * b).sum(axis=-1))
    return np.arctan2(s, d)
