"""Pins of tests/image_ref.py, the numpy restatement the GPU image ops are tested against: its colour functions
against the reference's own Color.h (oracle/_ref/libcf_ref.so), and its ops against the expectations of the
reference's lib/test/ImageTest.cpp cases that apply to an RGBAF image, re-stated case by case.  The same cases run
through cuttlefish_amd.Image on the GPU in tests/test_gpu_image_ops.py (make_image = its constructor)."""
import math

import numpy as np
import pytest

import image_ref as R
import oracle_lib as O

EPS = 1e-6            # ImageTestInfo(Image::Format::RGBAF, 1e-6, 4)
NORMAL_EPS = 1e-4


def _test_color(w, h, x, y):
    """getTestColor(image, x, y, divide=true)"""
    if x < w // 2:
        r, g = x / float(w - 1), y / float(h - 1)
    else:
        g, r = x / float(w - 1), y / float(h - 1)
    return [r, g, (x + y) / float(w + h - 2), (x + 2 * y) / float(w + 2 * h - 3)]


def _test_image(w, h):
    return np.array([[_test_color(w, h, x, y) for x in range(w)] for y in range(h)], np.float32)


def _expected(w, h):
    return np.array([[_test_color(w, h, x, y) for x in range(w)] for y in range(h)], np.float64)


def _close(got, want, eps, channels=4):
    assert np.all(np.abs(np.asarray(got, np.float64)[..., :channels] - want[..., :channels]) <= eps)


def case_flip_horizontal(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.flip_horizontal()
    _close(im.pixels, _expected(10, 15)[:, ::-1], EPS)


def case_flip_vertical(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.flip_vertical()
    _close(im.pixels, _expected(10, 15)[::-1], EPS)


def case_pre_multiply_alpha(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.pre_multiply_alpha()
    want = _expected(10, 15)
    want[..., :3] *= np.asarray(im.pixels, np.float64)[..., 3:4]
    _close(im.pixels, want, EPS)


def case_grayscale(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.grayscale()
    want = _expected(10, 15)
    want[..., :3] = R.to_grayscale(want[..., 0], want[..., 1], want[..., 2])[..., None]
    want[..., 3] = im.pixels[..., 3]
    _close(im.pixels, want, EPS)


def case_swizzle(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.swizzle(R.BLUE, R.RED, R.GREEN, R.ALPHA)
    t = _expected(10, 15)
    want = np.stack([t[..., 2], t[..., 0], t[..., 1], np.asarray(im.pixels, np.float64)[..., 3]], axis=-1)
    _close(im.pixels, want, EPS)


def case_linear_to_srgb(make_image):
    im = make_image(_test_image(10, 15), R.LINEAR)
    assert im.change_color_space(R.SRGB)
    assert im.color_space == R.SRGB
    want = R.linear_to_srgb(_expected(10, 15))
    want[..., 3] = im.pixels[..., 3]
    _close(im.pixels, want, EPS)


def case_srgb_to_linear(make_image):
    im = make_image(_test_image(10, 15), R.SRGB)
    assert im.change_color_space(R.LINEAR)
    assert im.color_space == R.LINEAR
    want = R.srgb_to_linear(_expected(10, 15))
    want[..., 3] = im.pixels[..., 3]
    _close(im.pixels, want, EPS)


def case_srgb_pre_multiply_alpha(make_image):
    im = make_image(_test_image(12, 16), R.SRGB)
    assert im.pre_multiply_alpha()
    assert im.color_space == R.SRGB
    t = _expected(12, 16)
    a = np.asarray(im.pixels, np.float64)[..., 3:4]
    want = t.copy()
    want[..., :3] = R.linear_to_srgb(R.srgb_to_linear(t[..., :3]) * a)
    _close(im.pixels, want, EPS)


def case_srgb_grayscale(make_image):
    im = make_image(_test_image(12, 16), R.SRGB)
    assert im.grayscale()
    assert im.color_space == R.SRGB
    t = R.srgb_to_linear(_expected(12, 16)[..., :3])
    want = _expected(12, 16)
    want[..., :3] = R.linear_to_srgb(R.to_grayscale(t[..., 0], t[..., 1], t[..., 2]))[..., None]
    _close(im.pixels, want, EPS)


def _height(w, h, x, y):
    """getHeight (ImageTest.cpp)"""
    return (x - w / 2.0) / (w / 2.0) * (y - h / 2.0) / (h / 2.0)


def _normal_case(make_image, options, keep_sign):
    n = 9
    src = np.zeros((n, n, 4), np.float32)
    for y in range(n):
        for x in range(n):
            src[y, x] = (_height(n, n, x, y), 0.0, 0.0, 1.0)
    im = make_image(src, R.LINEAR).create_normal_map(options, 2.5)
    wx, wy = options & R.WRAP_X, options & R.WRAP_Y
    for y in range(n):
        for x in range(n):
            x0 = _height(n, n, (n - 1 if wx else x) if x == 0 else x - 1, y)
            x1 = _height(n, n, (0 if wx else x) if x == n - 1 else x + 1, y)
            y0 = _height(n, n, x, (n - 1 if wy else y) if y == 0 else y - 1)
            y1 = _height(n, n, x, (0 if wy else y) if y == n - 1 else y + 1)
            width = 2.0 if wx else (1.0 if x == 0 or x == n - 1 else 2.0)
            height = 2.0 if wy else (1.0 if y == 0 or y == n - 1 else 2.0)
            dx = (x0 - x1) * 2.5 / width
            dy = (y1 - y0) * 2.5 / height
            length = math.sqrt(dx * dx + dy * dy + 1)
            want = np.array([dx / length, dy / length, 1.0 / length])
            got = np.asarray(im.pixels[y, x, :3], np.float64)
            if keep_sign:
                assert np.all((got >= -1.0) & (got <= 1.0))
            else:
                want = want * 0.5 + 0.5
                assert np.all((got >= 0.0) & (got <= 1.0))
            assert np.all(np.abs(got - want) <= NORMAL_EPS), (x, y, got, want)
    assert np.all(im.pixels[..., 3] == 1.0)


def case_normal_map(make_image):                  # NormalMapTest.CreateNormalMap (KeepSign)
    _normal_case(make_image, R.KEEP_SIGN, True)


def case_normal_map_keep_sign(make_image):        # NormalMapTest.CreateNormalMapKeepSign (Default options)
    _normal_case(make_image, 0, False)


def case_normal_map_wrap_x(make_image):
    _normal_case(make_image, R.WRAP_X, False)


def case_normal_map_wrap_y(make_image):
    _normal_case(make_image, R.WRAP_Y, False)


def _rotate_fallback(src, angle):
    """the fallback loops of Image::rotate (Image.cpp:1540-1597) in FreeImage's bottom-up scanlines: scanline y
    is numpy row h - 1 - y"""
    h, w = src.shape[:2]
    fi = src[::-1]                                   # fi[y] = scanline y
    if angle in (R.CCW90, R.CW270):
        out = np.zeros((w, h, 4), src.dtype)       # width h, height w
        for y in range(h):
            for x in range(w):
                out[x, h - y - 1] = fi[y, x]
    elif angle in (R.CCW180, R.CW180):
        out = np.zeros_like(src)
        for y in range(h):
            for x in range(w):
                out[h - y - 1, w - x - 1] = fi[y, x]
    else:
        out = np.zeros((w, h, 4), src.dtype)
        for y in range(h):
            for x in range(w):
                out[x, y] = fi[y, w - x - 1]
    return out[::-1]                                 # back to top-down rows


def case_rotate(make_image):                     # RotateFallbackTest.Rotate90: the mapping of the three angles
    src = _test_image(12, 16)
    for angle in range(6):
        got = make_image(src, R.LINEAR).rotate(angle)
        want = _rotate_fallback(src, angle)
        assert (got.width, got.height) == (want.shape[1], want.shape[0])
        assert np.array_equal(got.pixels, want), angle


CASES = [case_flip_horizontal, case_flip_vertical, case_pre_multiply_alpha, case_grayscale, case_swizzle,
         case_linear_to_srgb, case_srgb_to_linear, case_srgb_pre_multiply_alpha, case_srgb_grayscale,
         case_normal_map, case_normal_map_keep_sign, case_normal_map_wrap_x, case_normal_map_wrap_y, case_rotate]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_image_ref_matches_imagetest(case):
    case(R.RefImage)


def _sweep():
    """a dense sweep of [0, 1] with every float32 around the two knees"""
    v = [np.linspace(0.0, 1.0, 20001)]
    for knee in (0.04045, 0.0031308):
        k = np.float32(knee)
        around = k.view(np.int32) + np.arange(-2000, 2001, dtype=np.int32)
        v.append(around.view(np.float32).astype(np.float64))
        v.append(np.array([knee, np.nextafter(knee, 0.0), np.nextafter(knee, 1.0)]))
    v.append(np.arange(256) / 255.0)
    return np.concatenate(v)


def test_color_functions_match_color_h():
    ref = O.ref_lib()
    if ref is None:
        pytest.skip("oracle/_ref/libcf_ref.so not built (the reference's headers are absent)")
    c = _sweep()
    lin = R.srgb_to_linear(c)
    srgb = R.linear_to_srgb(c)
    for i in range(c.size):
        assert lin[i] == ref.cfref_srgb_to_linear(float(c[i])), c[i]
        assert srgb[i] == ref.cfref_linear_to_srgb(float(c[i])), c[i]
    rng = np.random.default_rng(5)
    rgb = rng.random((4000, 3))
    gray = R.to_grayscale(rgb[:, 0], rgb[:, 1], rgb[:, 2])
    for i in range(rgb.shape[0]):
        assert gray[i] == ref.cfref_to_grayscale(*map(float, rgb[i]))


def test_apply_ops_chains_the_single_ops():
    """apply_ops with several bits equals the single-op functions one after another (the order the GPU kernel
    fuses), an RGBF normal map included"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    got = R.apply_ops(a, 0xFF, R.SRGB, R.LINEAR, R.CW90, R.WRAP_X, 3.0, (R.ALPHA, R.RED, R.GREEN, R.BLUE))
    x = R.change_color_space(a, R.SRGB, R.LINEAR)
    x = R.grayscale(R.rotate(x, R.CW90), R.LINEAR)
    x = R.flip_vertical(R.flip_horizontal(R.normal_map(x, R.WRAP_X, 3.0)))
    x = R.pre_multiply_alpha(R.swizzle(x, (R.ALPHA, R.RED, R.GREEN, R.BLUE), True), R.LINEAR, True)
    assert got.shape == (5, 7, 4)
    assert np.array_equal(got, x)
    assert np.all(got[..., 3] == 1.0)
