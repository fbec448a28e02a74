"""numpy float64 restatement of cuttlefish::Image's pixel ops (lib/src/Image.cpp:1513-1882) -- the reference the GPU
image ops (csrc/image_ops.hip) are tested against.  Every op reads the RGBAF image as doubles and stores float
(astype(np.float32)) where the reference's setPixelNoGrayscaleImpl does.  Arrays are (h, w, 4), row 0 at the top.
Pinned to Color.h through oracle/_ref/libcf_ref.so and to ImageTest.cpp's expectations (tests/test_image_ref.py)."""
import math

import numpy as np

LINEAR, SRGB = 0, 1
CW90, CW180, CW270, CCW90, CCW180, CCW270 = range(6)
KEEP_SIGN, WRAP_X, WRAP_Y = 1, 2, 4
RED, GREEN, BLUE, ALPHA, NONE = range(5)


# libm's pow, as std::pow calls it: numpy's own vectorised power differs from it in the last bit
_pow = np.vectorize(math.pow, otypes=[np.float64])


def srgb_to_linear(c):
    """Color.h sRGBToLinear, elementwise in double"""
    c = np.asarray(c, np.float64)
    out = c / 12.92
    hi = c > 0.04045
    out[hi] = _pow((c[hi] + 0.055) / 1.055, 2.4)
    return out


def linear_to_srgb(c):
    """Color.h linearToSRGB, elementwise in double"""
    c = np.asarray(c, np.float64)
    out = c * 12.92
    hi = c > 0.0031308
    out[hi] = 1.055 * _pow(c[hi], 1.0 / 2.4) - 0.055
    return out


def to_grayscale(r, g, b):
    """Color.h toGrayscale (Rec. 709), in that operation order"""
    return r * 0.2126 + g * 0.7152 + b * 0.0722


def to_rgbaf(a):
    """Image::convert(RGBAF): uint8 as v/255.0, half floats as stored"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return (a.astype(np.float64) / 255.0).astype(np.float32)
    return a.astype(np.float32)


def change_color_space(a, src_cs, dst_cs):
    a = to_rgbaf(a).copy()
    if src_cs == dst_cs:
        return a
    f = srgb_to_linear if dst_cs == LINEAR else linear_to_srgb
    a[..., :3] = f(a[..., :3].astype(np.float64)).astype(np.float32)
    return a


def rotate(a, angle):
    """the fallback loops of Image::rotate: CCW90 = CW270 = np.rot90(a, 1), 180 = np.rot90(a, 2), CW90 = CCW270 = 3"""
    k = {CW90: 3, CW180: 2, CW270: 1, CCW90: 1, CCW180: 2, CCW270: 3}[angle]
    return np.ascontiguousarray(np.rot90(to_rgbaf(a), k))


def grayscale(a, cs):
    a = to_rgbaf(a).copy()
    c = a[..., :3].astype(np.float64)
    if cs == SRGB:
        c = srgb_to_linear(c)
    y = to_grayscale(c[..., 0], c[..., 1], c[..., 2])
    if cs == SRGB:
        y = linear_to_srgb(y)
    a[..., :3] = y.astype(np.float32)[..., None]
    return a


def normal_map(a, options, height):
    """Image::createNormalMap from the red channel -> an RGBF image (alpha 1)"""
    r = to_rgbaf(a)[..., 0].astype(np.float64)
    h, w = r.shape
    wx, wy = bool(options & WRAP_X), bool(options & WRAP_Y)
    xs = np.arange(w)
    ys = np.arange(h)
    left = (xs - 1) % w if wx else np.maximum(xs - 1, 0)
    right = (xs + 1) % w if wx else np.minimum(xs + 1, w - 1)
    up = (ys - 1) % h if wy else np.maximum(ys - 1, 0)
    down = (ys + 1) % h if wy else np.minimum(ys + 1, h - 1)
    dist_x = np.where(((xs == 0) | (xs == w - 1)) & (not wx), 1.0, 2.0)[None, :]
    dist_y = np.where(((ys == 0) | (ys == h - 1)) & (not wy), 1.0, 2.0)[:, None]
    dx = (r[:, left] - r[:, right]) * height / dist_x
    dy = (r[down, :] - r[up, :]) * height / dist_y
    length = np.sqrt(dx * dx + dy * dy + 1)
    n = np.stack([dx / length, dy / length, 1.0 / length], axis=-1)
    if not options & KEEP_SIGN:
        n = n * 0.5 + 0.5
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = n.astype(np.float32)
    return out


def flip_horizontal(a):
    return np.ascontiguousarray(to_rgbaf(a)[:, ::-1])


def flip_vertical(a):
    return np.ascontiguousarray(to_rgbaf(a)[::-1])


def swizzle(a, channels, rgbf=False):
    a = to_rgbaf(a).copy()
    if rgbf:
        a[..., 3] = 1.0
    out = np.empty_like(a)
    for i, c in enumerate(channels):
        out[..., i] = a[..., c] if c < 4 else (1.0 if i == 3 else 0.0)
    if rgbf:
        out[..., 3] = 1.0
    return out


def pre_multiply_alpha(a, cs, rgbf=False):
    """a no-op on an RGBF image: preMultiplyAlpha's switch has no RGBF case"""
    a = to_rgbaf(a).copy()
    if rgbf:
        a[..., 3] = 1.0
        return a
    c = a[..., :3].astype(np.float64)
    if cs == SRGB:
        c = srgb_to_linear(c)
    c = c * a[..., 3:4].astype(np.float64)
    if cs == SRGB:
        c = linear_to_srgb(c)
    a[..., :3] = c.astype(np.float32)
    return a


def apply_ops(a, ops, src_cs=LINEAR, dst_cs=None, rot=CW90, normal_options=0, normal_height=1.0,
              swz=(RED, GREEN, BLUE, ALPHA), rgbf=False):
    """one cfhip_image_ops_device call restated: the ops of the mask (ImageOp bit values) in the tool's order"""
    a = to_rgbaf(a).copy()
    if rgbf:
        a[..., 3] = 1.0
    cs = src_cs
    dst_cs = src_cs if dst_cs is None else dst_cs
    if ops & 1:
        a = change_color_space(a, cs, dst_cs)
        cs = dst_cs
    if ops & 2:
        a = rotate(a, rot)
    if ops & 4:
        a = grayscale(a, cs)
    if ops & 8:
        a = normal_map(a, normal_options, normal_height)
        rgbf = True
    if ops & 16:
        a = flip_horizontal(a)
    if ops & 32:
        a = flip_vertical(a)
    if ops & 64:
        a = swizzle(a, swz, rgbf)
    if ops & 128:
        a = pre_multiply_alpha(a, cs, rgbf)
    return a


class RefImage:
    """the numpy twin of cuttlefish_amd.Image: the same method names over the functions above"""

    def __init__(self, pixels, color_space=LINEAR, rgbf=False):
        self.pixels = to_rgbaf(pixels)
        self.color_space = color_space
        self.rgbf = rgbf

    @property
    def width(self):
        return self.pixels.shape[1]

    @property
    def height(self):
        return self.pixels.shape[0]

    def flip_horizontal(self):
        self.pixels = flip_horizontal(self.pixels)
        return True

    def flip_vertical(self):
        self.pixels = flip_vertical(self.pixels)
        return True

    def rotate(self, angle):
        return RefImage(rotate(self.pixels, angle), self.color_space, self.rgbf)

    def pre_multiply_alpha(self):
        self.pixels = pre_multiply_alpha(self.pixels, self.color_space, self.rgbf)
        return True

    def change_color_space(self, cs):
        self.pixels = change_color_space(self.pixels, self.color_space, cs)
        self.color_space = cs
        return True

    def grayscale(self):
        self.pixels = grayscale(self.pixels, self.color_space)
        return True

    def swizzle(self, r, g, b, a):
        self.pixels = swizzle(self.pixels, (r, g, b, a), self.rgbf)
        return True

    def create_normal_map(self, options=0, height=1.0):
        return RefImage(normal_map(self.pixels, options, height), self.color_space, True)
