"""The integrate's candidate test on d - z alone (the 8-byte staged record: the ray multiplier is gathered only by the
lanes that can update).  With m >= 1 and round-to-nearest monotone, (d - z) * m > -trunc implies d - z > -trunc, so
`cand = d - z > -trunc` is a superset of Open3D's update test and `cand & ((d - z) * m > -trunc)` is that test itself.
Checked here in float32 on the oracle's multiplier table of a wide camera (no GPU)."""
import numpy as np

WIDE_INTR = (64, 48, 32.0, 32.0, 31.5, 23.5)  # corner multiplier sqrt(1 + 0.75^2 + 1) = 1.6


def test_candidate_test_is_a_superset(O):
    mult = O.depth_multiplier(*WIDE_INTR)
    assert mult.dtype == np.float32
    assert (mult >= np.float32(1.0)).all()
    m = np.unique(mult)
    assert m.size > 100 and m.max() > np.float32(1.55)
    t = np.float32(0.04)  # (float)sdf_trunc, as the kernel's p.trunc
    grid = np.linspace(-2.0 * float(t), 0.0, 8001)[:-1].astype(np.float32)  # [-2 trunc, 0)
    edge = np.array([-t, np.nextafter(-t, np.float32(-1)), np.nextafter(-t, np.float32(0)),
                     np.float32(-2) * t, np.nextafter(np.float32(0), np.float32(-1))], np.float32)
    d = np.unique(np.concatenate([grid, edge]))
    assert d.dtype == np.float32 and (d < 0).all() and (d >= np.float32(-2) * t).all()
    prod = d[:, None] * m[None, :]  # float32 x float32: one IEEE rounding, as the kernel's v_mul_f32
    assert prod.dtype == np.float32
    assert (prod <= d[:, None]).all(), "RN(diff * m) <= diff for diff < 0, m >= 1"
    upd = prod > -t            # Open3D's test on the scaled distance
    cand = (d > -t)[:, None]   # the candidate test on the difference alone
    assert not (upd & ~cand).any(), "an updating lane would not have been a candidate"
    gap = cand & ~upd
    assert gap.any(), "no pair with diff > -trunc >= diff * m: the gap between the two tests is not exercised"
    # for diff >= 0 the update test passes whatever the multiplier (and so does the candidate test)
    dp = np.abs(d)
    assert ((dp[:, None] * m[None, :]) > -t).all() and (dp > -t).all()
