"""numpy twin of alpha bleeding (include/cuttlefish_hip.h: cfhip_alpha_bleed_array_device),
written from the definition alone: every texel whose alpha is not above the threshold takes the R, G, B storage bits of
the seed a jump flood finds for it.  The twin is the definition: the kernels return its bytes and its record.

bleed(image, ...) takes and returns an (h, w, 4) uint8 / float16 / float32 array and the record of the surface."""
import numpy as np

WRAP_X, WRAP_Y = 1, 2
NONE = 0xFFFFFFFF
FIELDS = ("seeds", "filled", "max_dist2", "reserved")
_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def alpha_of(image: np.ndarray) -> np.ndarray:
    """alpha as float32: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored"""
    a = np.asarray(image)[..., 3]
    if a.dtype == np.uint8:
        return (a.astype(np.float64)/255.0).astype(np.float32)
    if a.dtype in (np.float16, np.float32):
        return a.astype(np.float32)
    raise TypeError("pixel dtype %s" % a.dtype)


def seed_mask(image: np.ndarray, threshold=0.0) -> np.ndarray:
    """texels with alpha > threshold, compared in float32; a NaN alpha is not a seed"""
    with np.errstate(invalid="ignore"):
        return alpha_of(image) > np.float32(threshold)


def steps_of(width: int, height: int):
    """P/2, P/4, ..., 1 and one more 1, P the smallest power of two >= max(width, height); [1] for 1 x 1"""
    p = 1
    while p < max(width, height):
        p *= 2
    steps = []
    k = p//2
    while k >= 1:
        steps.append(k)
        k //= 2
    return steps + [1]


def dist2(x, y, words, width: int, height: int, wrap_x: bool, wrap_y: bool) -> np.ndarray:
    """d^2 between the texels (x, y) and the seeds named by `words` (which must not be NONE), as uint64"""
    sx = (words & np.uint32(0xFFFF)).astype(np.int64)
    sy = (words >> np.uint32(16)).astype(np.int64)
    dx = np.abs(x - sx)
    dy = np.abs(y - sy)
    if wrap_x:
        dx = np.minimum(dx, width - dx)
    if wrap_y:
        dy = np.minimum(dy, height - dy)
    return (dx*dx + dy*dy).astype(np.uint64)


def _keys(x, y, words, width, height, wrap_x, wrap_y):
    """d^2 << 32 | seed word per texel; no seed: the largest key"""
    have = words != np.uint32(NONE)
    safe = np.where(have, words, np.uint32(0))
    key = (dist2(x, y, safe, width, height, wrap_x, wrap_y) << np.uint64(32)) | safe.astype(np.uint64)
    return np.where(have, key, _NO_KEY)


def jump_flood(mask: np.ndarray, wrap_x: bool = False, wrap_y: bool = False, steps=None):
    """-> (seed word per texel, NONE where none; its d^2 as uint64, undefined where none) after pass 0 and the steps
    (steps_of by default)."""
    h, w = mask.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    words = np.where(mask, (x | (y << 16)).astype(np.uint32), np.uint32(NONE))
    best = _keys(x, y, words, w, h, wrap_x, wrap_y)
    for k in (steps_of(w, h) if steps is None else steps):
        best = np.full((h, w), _NO_KEY, np.uint64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                px, py = x + k*dx, y + k*dy
                inside = np.ones((h, w), bool)
                if wrap_x:
                    px = px % w
                else:
                    inside &= (px >= 0) & (px < w)
                if wrap_y:
                    py = py % h
                else:
                    inside &= (py >= 0) & (py < h)
                cand = words[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)]      # read from the previous pass's buffer
                cand = np.where(inside, cand, np.uint32(NONE))
                best = np.minimum(best, _keys(x, y, cand, w, h, wrap_x, wrap_y))
        words = (best & np.uint64(NONE)).astype(np.uint32)                     # the largest key's low word is NONE
    return words, best >> np.uint64(32)


def exact_nearest(mask: np.ndarray, wrap_x: bool = False, wrap_y: bool = False):
    """brute force: the seed of minimal key over all seeds per texel -> (words, d^2); for the tests of the flood"""
    h, w = mask.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    sy, sx = np.nonzero(mask)
    if sx.size == 0:
        return np.full((h, w), NONE, np.uint32), np.zeros((h, w), np.uint64)
    seeds = (sx | (sy << 16)).astype(np.uint32)
    key = _keys(x[..., None], y[..., None], seeds[None, None, :], w, h, wrap_x, wrap_y).min(-1)
    return (key & np.uint64(NONE)).astype(np.uint32), key >> np.uint64(32)


def bleed(image: np.ndarray, threshold=0.0, wrap=(False, False), max_distance: int = 0):
    """-> (the bled image, {"seeds", "filled", "max_dist2", "reserved"}).  wrap: a bool for both axes or (x, y)."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 4 or image.dtype not in (np.uint8, np.float16, np.float32):
        raise TypeError("expected an (h, w, 4) uint8 / float16 / float32 image")
    if not (0.0 <= float(threshold) < 1.0) or not (0 <= int(max_distance) <= 65535):
        raise ValueError("threshold in [0, 1), max_distance in 0 .. 65535")
    wrap_x, wrap_y = (bool(wrap), bool(wrap)) if isinstance(wrap, (bool, np.bool_)) else (bool(wrap[0]), bool(wrap[1]))
    mask = seed_mask(image, threshold)
    words, d2 = jump_flood(mask, wrap_x, wrap_y)
    fill = ~mask & (words != np.uint32(NONE))
    if max_distance:
        fill &= d2 <= np.uint64(int(max_distance)**2)
    out = image.copy()
    sx = (words & np.uint32(0xFFFF)).astype(np.int64)
    sy = (words >> np.uint32(16)).astype(np.int64)
    bits = out.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[image.dtype.itemsize])    # storage bits, no arithmetic
    src = image.view(bits.dtype)
    bits[fill, :3] = src[sy[fill], sx[fill], :3]
    rec = {"seeds": int(mask.sum()), "filled": int(fill.sum()), "max_dist2": int(d2[fill].max()) if fill.any() else 0,
           "reserved": 0}
    return out, rec
