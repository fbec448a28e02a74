"""The ranges csrc/bc7_rcp.h leans on, on the CPU: the arguments of the three reciprocals that run without a test lie
inside the binades on which v_rcp_f32 and one Newton step equal the division (biased exponent 2..252, swept on the
device by tools/ubench/rcp_sweep.hip), and so does every 1/mx the kernel can form.

  64 det       det = n C - S^2 over every selector multiset is at least 1 where it is positive and at most 16 * 16 * 64^2
  sqrt(l2),    an axis divided by its largest magnitude, in float32 with the kernel's operation order: 2^20 seeded axes
  den          over 60 binades of mx, and the corner cases (one component, all components equal, the extremes of mx)
  mx           at most 2^24 * (4 * 2^24)^3 = 2^102 and, as a sum of integer-valued floats, at least 1 when positive
"""
import numpy as np

F = np.float32


def _biased_exponent(x):
    return (np.asarray(x, F).view(np.uint32) >> 23) & 255


def test_det_range():
    lo, hi = F(64.0)*F(1), F(64.0)*F(16*16*4096)
    assert _biased_exponent(lo) == 133 and _biased_exponent(hi) == 153
    # det is an integer below 2^24: its float is exact, and so is the product with 64
    assert 16*16*4096 < 1 << 24


def test_mx_range():
    top = F(2.0)**F(24)*(F(4.0)*F(2.0)**F(24))**F(3)
    assert top == F(2.0)**F(102) and _biased_exponent(top) == 229 and _biased_exponent(F(1.0)) == 127
    # a covariance term n q - s s of 16 texels of bytes stays below 2^24: an exact float
    assert 16*16*255*255 < 1 << 24


def _l2(v):
    """the kernel's order: im = 1/mx, v*im, l2 = v0*v0 then three fused multiply-adds (float64 holds a float32 product
    exactly, so rounding its sum once is the fused operation)"""
    mx = np.max(np.abs(v), axis=1).astype(F)
    im = (F(1.0)/mx).astype(F)
    w = (v*im[:, None]).astype(F)
    l2 = (w[:, 0]*w[:, 0]).astype(F)
    for c in (1, 2, 3):
        l2 = (w[:, c].astype(np.float64)*w[:, c].astype(np.float64) + l2.astype(np.float64)).astype(F)
    return l2


def test_l2_and_den_range():
    r = np.random.default_rng(5)
    v = r.standard_normal((1 << 20, 4)).astype(F)*np.exp2(r.integers(0, 60, (1 << 20, 1))).astype(F)
    corners = []
    for mag in (1.0, 3.0, 16777215.0, 2.0**102, 2.0**101*1.9999999):
        corners += [[mag, 0, 0, 0], [mag, mag, mag, mag], [mag, -mag, mag*0.99999994, 0], [0, 0, 0, -mag]]
    l2 = _l2(np.concatenate([v, np.array(corners, F)]))
    assert l2.min() > 1.0 - 2.0**-21 and l2.max() < 4.0 + 2.0**-20, (l2.min(), l2.max())
    root = np.sqrt(l2.astype(np.float64)).astype(F)
    for x in (l2, root):
        e = _biased_exponent(x)
        assert e.min() >= 126 and e.max() <= 129, (e.min(), e.max())
