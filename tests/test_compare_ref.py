"""The numpy restatement of the quality metrics (tests/compare_ref.py) against closed forms and against an
independent SSIM built on scipy.ndimage.  CPU only."""
import numpy as np
import pytest

import compare_ref as R
from cuttlefish_amd.api import Layout


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def test_identical_images_give_zero_sse_and_unit_ssim():
    ref = _img(23, 31, 1)
    out = R.compare(ref, Layout.RGBA8, ref, (4, 4), ssim=True)
    assert out["sse"] == [0.0] * 4
    assert out["ssim"] == pytest.approx([1.0] * 4, abs=1e-12)
    assert out["windows"] == 13 * 21
    assert out["channels"] == 15
    assert np.all(out["block_errors"] == 0.0)


def _constant_ssim(x, y, rng):
    """closed form for constant images x, y: the luminance term (2 mx my + C1) / (mx^2 + my^2 + C1).  The taps are
    rounded to float, so the window weights sum to S = 1 + O(1e-8) and the variances S x^2 - (S x)^2 do not quite
    vanish: they are kept, exactly."""
    S = float(R.gaussian_taps().sum()) ** 2
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    mx, my = S * x, S * y
    vx, vy, cxy = S * x * x - mx * mx, S * y * y - my * my, S * x * y - mx * my
    assert abs(S - 1.0) < 1e-6
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def test_constant_against_constant_offset_is_the_luminance_term():
    h, w = 20, 17
    dec = np.full((h, w, 1), 200, np.uint8)
    ref = np.zeros((h, w, 4), np.uint8)
    ref[..., 0] = 150
    out = R.compare(dec, Layout.R8, ref, (4, 4), ssim=True)
    x, y = 200 / 255.0, 150 / 255.0
    c1 = 0.01 ** 2
    assert out["ssim"][0] == pytest.approx(_constant_ssim(x, y, 1.0), abs=1e-12)
    assert out["ssim"][0] == pytest.approx((2 * x * y + c1) / (x * x + y * y + c1), abs=1e-5)
    assert out["sse"][0] == pytest.approx(h * w * (x - y) ** 2, rel=1e-12)
    assert out["channels"] == 1 and np.isnan(out["ssim"][1])


def test_snorm_constant_uses_range_two():
    dec = np.full((12, 12, 2), -64, np.int8)
    ref = np.zeros((12, 12, 4), np.float32)
    ref[..., 0] = 0.25
    ref[..., 1] = -0.75
    out = R.compare(dec, Layout.RG8_SNorm, ref, (4, 4), ssim=True)
    x = -64 / 127.0
    for c, y in ((0, 0.25), (1, -0.75)):
        assert out["ssim"][c] == pytest.approx(_constant_ssim(x, y, 2.0), abs=1e-12)
    assert R.normalise(np.array([-128], np.int8), Layout.R8_SNorm)[0] == -1.0


def test_ssim_matches_scipy_gaussian_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    x = rng.random((40, 53))
    y = np.clip(x + 0.1 * rng.standard_normal(x.shape), 0, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def g(a):
        return ndimage.gaussian_filter(a, 1.5, truncate=10.0 / 3.0, mode="constant")[5:-5, 5:-5]
    mx, my = g(x), g(y)
    vx, vy, cxy = g(x * x) - mx * mx, g(y * y) - my * my, g(x * y) - mx * my
    want = (((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()
    assert R.ssim_channel(x, y, 1.0) == pytest.approx(want, abs=1e-6)


def test_ssim_is_nan_below_eleven():
    ref = _img(10, 40, 3)
    out = R.compare(ref, Layout.RGBA8, ref, (4, 4), ssim=True)
    assert all(np.isnan(v) for v in out["ssim"]) and out["windows"] == 0


def test_block_sums_add_up_to_total_sse():
    ref = _img(37, 61, 4)
    dec = _img(37, 61, 5)
    out = R.compare(dec, Layout.RGBA8, ref, (6, 5), mask=(True, False, True, True))
    assert out["block_errors"].shape == (8, 11)
    assert out["block_errors"].sum() == pytest.approx(sum(out["sse"]), rel=1e-12)
    assert out["sse"][1] == 0.0 and out["channels"] == 0b1101


def test_hdr_log_sse_and_ref_max():
    rng = np.random.default_rng(9)
    ref = (rng.random((8, 8, 4)) * 10).astype(np.float16)
    dec = (ref.astype(np.float32) * 1.5).astype(np.float16)
    dec[0, 0, 0] = 0.0                         # clamps to 2^-24
    out = R.compare(dec, Layout.RGBA16F, ref, (4, 4), ssim=True)
    r = ref.astype(np.float64)
    lg = np.log2(np.maximum(dec.astype(np.float64), 2.0 ** -24)) - np.log2(np.maximum(r, 2.0 ** -24))
    assert out["log_sse"] == pytest.approx([(lg[..., c] ** 2).sum() for c in range(4)], rel=1e-12)
    assert out["ref_max"] == [float(r[..., c].max()) for c in range(4)]
    assert all(np.isnan(v) for v in out["ssim"])
