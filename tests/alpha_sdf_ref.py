"""numpy twin of the signed distance field from alpha (include/cuttlefish_hip.h: cfhip_alpha_sdf_array_device; DESIGN.md
section 4.22), written from the definition alone: classes from alpha, the Euclidean distance between texel centres to the
nearest texel of the other class capped at K = spread + 1, signed, averaged over s x s tiles, stored with 0.5 at the
silhouette.  The twin is the definition: the kernels return its bytes and its record.

squared_distance() is the windowed two-pass form (a row pass, then a min-plus column pass over |dy| < K);
tests/test_alpha_sdf_ref.py holds it to the brute-force minimum over all pairs.

sdf(image, spread, ...) takes an (h, w, 4) uint8 / float16 / float32 array and returns the (h/s, w/s) values as stored in
out_dtype and the record of the surface; apply() writes them into the named channels of a destination."""
import numpy as np

WRAP_X, WRAP_Y = 1, 2
FIELDS = ("inside", "saturated", "reserved0", "reserved1")
SCALES = (1, 2, 4, 8, 16)
MAX_SPREAD = 126
CHANNEL_BITS = {"r": 1, "g": 2, "b": 4, "a": 8}


def alpha_of(image: np.ndarray) -> np.ndarray:
    """alpha as float32: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored"""
    a = np.asarray(image)[..., 3]
    if a.dtype == np.uint8:
        return (a.astype(np.float64)/255.0).astype(np.float32)
    if a.dtype in (np.float16, np.float32):
        return a.astype(np.float32)
    raise TypeError("pixel dtype %s" % a.dtype)


def inside_mask(image: np.ndarray, threshold=0.5) -> np.ndarray:
    """texels with alpha > threshold, compared in float32; a NaN alpha is outside"""
    with np.errstate(invalid="ignore"):
        return alpha_of(image) > np.float32(threshold)


def wrap_axes(wrap):
    if isinstance(wrap, (bool, np.bool_)):
        return bool(wrap), bool(wrap)
    x, y = wrap
    return bool(x), bool(y)


def channel_mask(channels) -> int:
    """"a", "rgba", "gb", ... -> the bits R = 1, G = 2, B = 4, A = 8"""
    if isinstance(channels, (int, np.integer)):
        return int(channels)
    mask = 0
    for ch in channels:
        mask |= CHANNEL_BITS[ch.lower()]
    return mask


def _shifted(a: np.ndarray, d: int, axis: int, wrap: bool, fill):
    """b[i] = a[i + d] along the axis: modulo the size with wrap, `fill` outside without"""
    n = a.shape[axis]
    if wrap:
        return np.roll(a, -d, axis)
    out = np.full_like(a, fill)
    if abs(d) >= n:
        return out
    src = [slice(None)]*a.ndim
    dst = [slice(None)]*a.ndim
    src[axis] = slice(max(d, 0), n + min(d, 0))
    dst[axis] = slice(max(-d, 0), n - max(d, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def row_distance(mask: np.ndarray, spread: int, wrap_x: bool) -> np.ndarray:
    """per texel the distance to the nearest texel of the other class in its row, capped at K"""
    k = spread + 1
    cls = mask.astype(np.int8)
    g = np.full(mask.shape, k, np.int64)
    for d in range(k - 1, 0, -1):
        for sd in (d, -d):
            other = _shifted(cls, sd, 1, wrap_x, -1)
            g[(other >= 0) & (other != cls)] = d
    return g


def squared_distance(mask: np.ndarray, spread: int, wrap=False) -> np.ndarray:
    """e = min(K^2, min dx^2 + dy^2 over the texels of the other class) as int64: the row distances, then per texel the
    minimum over |dy| < K of dy^2 + g^2, g = 0 where that row's texel is of the other class, its row distance where
    that is below K, no candidate otherwise"""
    wx, wy = wrap_axes(wrap)
    k = spread + 1
    cls = np.asarray(mask, bool).astype(np.int8)
    g = row_distance(cls.astype(bool), spread, wx)
    e = np.full(cls.shape, k*k, np.int64)
    for dy in range(-(k - 1), k):
        c2 = _shifted(cls, dy, 0, wy, -1)
        g2 = _shifted(g, dy, 0, wy, k)
        cand = np.where(c2 != cls, dy*dy, np.where(g2 < k, dy*dy + g2*g2, k*k))
        e = np.where(c2 >= 0, np.minimum(e, cand), e)
    return e


def signed_distance(e: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """rho = (float)sqrt((double)e); rho - 0.5 inside, 0.5 - rho outside, as float64 (exact)"""
    rho = np.sqrt(e.astype(np.float64)).astype(np.float32).astype(np.float64)
    return np.where(mask, rho - 0.5, 0.5 - rho)


def tile_mean(sd: np.ndarray, scale: int) -> np.ndarray:
    h, w = sd.shape
    return sd.reshape(h//scale, scale, w//scale, scale).sum((1, 3))/float(scale*scale)


def value(m: np.ndarray, spread: int) -> np.ndarray:
    """v = 0.5 + m / (2.0 * spread) in double, clamped to [0, 1]"""
    return np.clip(0.5 + m/(2.0*spread), 0.0, 1.0)


def quantise(v: np.ndarray, dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.floor(v*255.0 + 0.5).astype(np.uint8)
    if dtype == np.float32:
        return v.astype(np.float32)
    if dtype == np.float16:
        return v.astype(np.float32).astype(np.float16)
    raise TypeError("pixel dtype %s" % dtype)


def field_of_mask(mask: np.ndarray, spread: int, scale: int = 1, wrap=False):
    """-> (v as float64 (h/s, w/s), e)"""
    h, w = mask.shape
    if scale not in SCALES or h % scale or w % scale or not 1 <= spread <= MAX_SPREAD:
        raise ValueError("scale %r, spread %r, %dx%d" % (scale, spread, w, h))
    e = squared_distance(mask, spread, wrap)
    return value(tile_mean(signed_distance(e, mask), scale), spread), e


def sdf(image: np.ndarray, spread: int, scale: int = 1, threshold=0.5, wrap=False, out_dtype=None):
    """-> (the stored values (h/s, w/s) of out_dtype -- the image's by default --, the record as a dict)"""
    image = np.asarray(image)
    mask = inside_mask(image, threshold)
    v, e = field_of_mask(mask, spread, scale, wrap)
    k = spread + 1
    rec = dict(inside=int(mask.sum()), saturated=int((e == k*k).sum()), reserved0=0, reserved1=0)
    return quantise(v, image.dtype if out_dtype is None else out_dtype), rec


def apply(dst: np.ndarray, values: np.ndarray, channels="a") -> np.ndarray:
    """a copy of dst (H, W, 4) with the values in the channels of the mask, the others as they were"""
    out = np.array(dst, copy=True)
    mask = channel_mask(channels)
    for ch in range(4):
        if mask >> ch & 1:
            out[..., ch] = values
    return out


def brute_force(mask: np.ndarray, spread: int, wrap=False) -> np.ndarray:
    """e by the definition's own words: the minimum over all pairs of texels of different classes (small masks only)"""
    wx, wy = wrap_axes(wrap)
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    k = spread + 1
    y, x = np.mgrid[0:h, 0:w]
    x, y, c = x.ravel(), y.ravel(), mask.ravel()
    dx = np.abs(x[:, None] - x[None, :])
    dy = np.abs(y[:, None] - y[None, :])
    if wx:
        dx = np.minimum(dx, w - dx)
    if wy:
        dy = np.minimum(dy, h - dy)
    d2 = np.where(c[:, None] != c[None, :], dx*dx + dy*dy, k*k)
    return np.minimum(d2.min(1), k*k).reshape(h, w).astype(np.int64)


# ---- the magnification condition: three 256^2 masks, their field at scale 8 magnified bilinearly by 8 ---------------
def shapes(n: int = 256):
    """{name: bool (n, n)}: an off-centre disc, a slanted bar, a five-lobed star"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) + 0.5
    s = n/256.0
    disc = (x - 117.3*s)**2 + (y - 139.6*s)**2 <= (71.4*s)**2
    t = np.deg2rad(27.0)
    u = (x - n/2)*np.cos(t) + (y - n/2)*np.sin(t)
    v = -(x - n/2)*np.sin(t) + (y - n/2)*np.cos(t)
    bar = (np.abs(u) <= 96.0*s) & (np.abs(v) <= 23.0*s)
    ang = np.arctan2(y - 126.2*s, x - 130.7*s)
    r = np.hypot(x - 130.7*s, y - 126.2*s)
    star = r <= (62.0 + 34.0*np.cos(5.0*ang + 0.4))*s
    return {"disc": disc, "bar": bar, "star": star}


def magnify(low: np.ndarray, factor: int) -> np.ndarray:
    """bilinear magnification as a sampler does it: texel centres at i + 0.5, coordinates clamped to the edge"""
    def taps(n):
        u = (np.arange(n*factor) + 0.5)/factor - 0.5
        i0 = np.floor(u).astype(np.int64)
        f = u - i0
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f
    low = low.astype(np.float64)
    y0, y1, fy = taps(low.shape[0])
    x0, x1, fx = taps(low.shape[1])
    top = low[y0][:, x0]*(1 - fx) + low[y0][:, x1]*fx
    bot = low[y1][:, x0]*(1 - fx) + low[y1][:, x1]*fx
    return top*(1 - fy)[:, None] + bot*fy[:, None]


def mismatches(low: np.ndarray, mask: np.ndarray) -> int:
    """texels of the mask that a 0.5 threshold of the magnified low-resolution values gets wrong"""
    factor = mask.shape[0]//low.shape[0]
    return int(((magnify(low, factor) > 0.5) != mask).sum())


def box_alpha(mask: np.ndarray, scale: int) -> np.ndarray:
    """the yardstick: the mask's alpha (0 / 255) box-filtered to 1 / scale, as 8 bits"""
    h, w = mask.shape
    mean = mask.reshape(h//scale, scale, w//scale, scale).mean((1, 3))
    return np.floor(mean*255.0 + 0.5).astype(np.uint8)/255.0
