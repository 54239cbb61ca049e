"""The designed clouds of the segment_plane tests (none above 5 000 points).  test_segment_plane_api.py asserts on the
numpy reference alone that each has the property it was built for; test_gpu_segment_plane.py runs them on the GPU."""
import numpy as np


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q if np.linalg.det(q) > 0 else -q


def plane_and_noise(seed, n, frac, thickness=0.004, extent=1.0, offset=(0.0, 0.0, 0.0)):
    """round(frac n) points within `thickness` of a randomly rotated plane patch, the rest uniform in the box around
    it, shuffled; signed coordinates"""
    rng = np.random.default_rng(seed)
    m = int(round(frac * n))
    patch = np.column_stack([rng.uniform(-extent, extent, m), rng.uniform(-extent, extent, m),
                             rng.uniform(-thickness, thickness, m)])
    pts = np.concatenate([patch @ rotation(rng).T, rng.uniform(-extent, extent, (n - m, 3))])
    pts = pts[rng.permutation(n)] + rng.uniform(-0.3, 0.3, 3)
    return np.ascontiguousarray(pts + np.asarray(offset, np.float64))


THRESHOLD = 0.01  # for plane_and_noise clouds: above the patch's thickness

# (ransac_n, num_iterations) of the random-cloud cases; 255 / 256 / 257 straddle the GPU's chunk of 256 iterations
RANDOM_PARAMS = [(3, 1), (3, 63), (3, 65), (3, 100), (3, 255), (3, 256), (3, 257), (3, 1000), (4, 100), (6, 100)]


def random_cases():
    """(name, points, threshold, ransac_n, num_iterations, probability, seed)"""
    out = []
    for j, (rn, iters) in enumerate(RANDOM_PARAMS):
        # a thin plane share keeps the break threshold above the iteration count, a large one breaks early
        frac = (0.3, 0.55, 0.8)[j % 3]
        n = (1000, 1777, 2500)[(j // 3) % 3]
        out.append((f"random n={n} frac={frac} ransac_n={rn} iters={iters}", plane_and_noise(100 + j, n, frac),
                    THRESHOLD, rn, iters, 0.99999999, 7 + j))
    return out


def long_run_cases():
    """low plane shares with many iterations: the loop runs through several chunks before it breaks, or never breaks"""
    return [("20 % plane, 1000 iterations", plane_and_noise(131, 1500, 0.2), THRESHOLD, 3, 1000, 0.99999999, 3),
            ("15 % plane, 600 iterations", plane_and_noise(132, 1200, 0.15), THRESHOLD, 3, 600, 0.99999999, 4)]


def size_cases():
    """N = 3, 4 (less than a wave), 65 (a wave plus one), 257 (a workgroup plus one), 4097 (more than one chain chunk
    of inliers, signed coordinates)"""
    out = [("N=3", np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -0.5]]), 0.01, 3),
           ("N=4", np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -0.5], [1.0, 1.0, -0.25]]), 0.01, 4)]
    for n in (65, 257, 4097):
        out.append((f"N={n}", plane_and_noise(200 + n, n, 0.7), THRESHOLD, 3))
    return out


def lattice(nx, ny, z=0.0, x0=0, y0=0):
    gx, gy = np.meshgrid(np.arange(nx) + x0, np.arange(ny) + y0, indexing="ij")
    return np.column_stack([gx.ravel(), gy.ravel(), np.full(nx * ny, z)]).astype(np.float64)


SLAB_THRESHOLD = 0.05


def slabs_exact_and_jittered(seed=301):
    """two 12 x 12 slabs of equal inlier count: z = 0 on the integer lattice (every candidate from it has err exactly
    0) and z = 3 with +-1e-4 of jitter (err > 0), interleaved so that either can come first: rmse decides"""
    rng = np.random.default_rng(seed)
    a = lattice(12, 12, 0.0)
    b = lattice(12, 12, 3.0, x0=20)
    b[:, 2] += rng.uniform(-1e-4, 1e-4, len(b))
    pts = np.concatenate([a, b])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def slabs_both_exact(seed=302):
    """two exact lattice slabs of equal count (z = 0 and z = 3): every full-count candidate has rmse 0, the earliest
    one wins"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([lattice(12, 12, 0.0), lattice(12, 12, 3.0, x0=20)])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def at_threshold(seed=303):
    """a 20 x 20 lattice at z = 0 and 16 points each at z = +0.25 and z = -0.25 above it: against the lattice plane
    these are at exactly 0.25.  Returns (points, indices of the raised points)"""
    rng = np.random.default_rng(seed)
    base = lattice(20, 20, 0.0)
    up = lattice(4, 4, 0.25, x0=3, y0=5)
    down = lattice(4, 4, -0.25, x0=12, y0=9)
    pts = np.concatenate([base, up, down])
    perm = rng.permutation(len(pts))
    pts = np.ascontiguousarray(pts[perm])
    raised = np.nonzero(pts[:, 2] != 0.0)[0]
    return pts, raised


def degenerate(seed=304):
    """300 copies of one point, 150 points on one line and a 6 x 6 lattice patch: most samples are coincident or
    collinear and give the zero plane"""
    rng = np.random.default_rng(seed)
    same = np.tile([[2.0, -1.0, 0.5]], (300, 1))
    t = np.arange(150, dtype=np.float64)[:, None]
    line = np.array([[2.0, -1.0, 0.5]]) + t * np.array([[1.0, 2.0, -1.0]])
    patch = lattice(6, 6, 4.0, x0=-10, y0=-10)
    pts = np.concatenate([same, line, patch])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def one_plane():
    """every point on the exact plane z = 2: fitness 1, the loop stops after the first counted candidate"""
    return lattice(25, 20, 2.0, x0=-7, y0=-3)


def offset_cloud():
    return plane_and_noise(305, 2000, 0.6, offset=(1000.0, -2000.0, 500.0))
