"""numpy twin of the mip post-pass (include/cuttlefish_hip.h: cfhip_mip_post_array_device),
written from the definitions alone: coverage is an integer count of texels with fl32(alpha * s) >= t, the scale of a
level is an extremum over float32 bit patterns found here by plain bisection, normals are renormalised in double.

post(level0, levels, ...) takes and returns (h, w, 4) arrays and the result records."""
import numpy as np

S_MIN, S_MAX = np.float32(0.25), np.float32(4.0)
COVERAGE, NORMALIZE, SIGNED_NORMALS = 1, 2, 4
FIELDS = ("scale", "target", "count_before", "count_after")


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def fl(b: int) -> np.float32:
    return np.uint32(b).view(np.float32)


ONE = bits(1.0)


def alpha_of(image: np.ndarray) -> np.ndarray:
    """alpha as float32: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored"""
    a = np.asarray(image)[..., 3]
    if a.dtype == np.uint8:
        return (a.astype(np.float64)/255.0).astype(np.float32)
    if a.dtype in (np.float16, np.float32):
        return a.astype(np.float32)
    raise TypeError("pixel dtype %s" % a.dtype)


def count(alpha: np.ndarray, s, t) -> int:
    """texels with fl32(alpha * s) >= t; NaN and negative alphas never count"""
    with np.errstate(all="ignore"):
        return int(np.count_nonzero(alpha.astype(np.float32)*np.float32(s) >= np.float32(t)))


def coverage(image: np.ndarray, t, s=1.0) -> int:
    return count(alpha_of(image), s, t)


def target(c0: int, n_k: int, n_0: int) -> int:
    return (int(c0)*int(n_k) + int(n_0)//2)//int(n_0)


def search(alpha: np.ndarray, T: int, t):
    """rules 1-5 -> (scale, count_before, count_after, how); how names the rule that chose, for the tests:
    'same', 'u', 'd', 'max', 'min', suffixed '=1' when rule 5 put the scale back to 1"""
    cnt = lambda b: count(alpha, fl(b), t)         # noqa: E731
    c1 = cnt(ONE)
    if c1 == T:
        return np.float32(1), c1, c1, "same"
    if c1 < T:
        lo, hi = ONE, bits(S_MAX)
        if cnt(hi) < T:
            cands = [("max", hi)]
        else:
            while hi - lo > 1:
                mid = (lo + hi)//2
                if cnt(mid) >= T:
                    hi = mid
                else:
                    lo = mid
            cands = [("u", hi), ("d", hi - 1)]
    else:
        lo, hi = bits(S_MIN), ONE
        if cnt(lo) > T:
            cands = [("min", lo)]
        else:
            while hi - lo > 1:
                mid = (lo + hi)//2
                if cnt(mid) <= T:
                    lo = mid
                else:
                    hi = mid
            cands = [("u", lo + 1), ("d", lo)]
    how, p = cands[0]
    if len(cands) == 2 and abs(cnt(cands[0][1]) - T) > abs(cnt(cands[1][1]) - T):
        how, p = cands[1]
    c = cnt(p)
    if c == c1:
        return np.float32(1), c1, c1, how + "=1"
    return fl(p), c1, c, how


def scale_alpha(level: np.ndarray, s) -> np.ndarray:
    """s != 1: alpha = fminf(fl32(alpha * s), 1.0f); s == 1: the level as it was"""
    out = np.array(level, dtype=np.float32, copy=True)
    if np.float32(s) != np.float32(1):
        with np.errstate(all="ignore"):
            out[..., 3] = np.fmin(out[..., 3]*np.float32(s), np.float32(1))
    return out


def normalize(level: np.ndarray, signed: bool) -> np.ndarray:
    out = np.array(level, dtype=np.float32, copy=True)
    with np.errstate(all="ignore"):
        v = out[..., :3].astype(np.float64)
        if not signed:
            v = v*2.0 - 1.0
        x, y, z = v[..., 0], v[..., 1], v[..., 2]
        length = np.sqrt((x*x + y*y) + z*z)
        ok = np.isfinite(length) & (length > 0)
        n = v/np.where(ok, length, 1.0)[..., None]
        n[~ok] = (0.0, 0.0, 1.0)
        if not signed:
            n = n*0.5 + 0.5
        out[..., :3] = n.astype(np.float32)
    return out


def post(level0: np.ndarray, levels, flags: int, t=0.5, info=None):
    """One chain: level0 (h, w, 4) of uint8 / float16 / float32, levels = its float32 levels 1.. -> (the levels after the
    pass, the records as dicts -- [] without COVERAGE).  info, if a list, receives search()'s `how` per level."""
    out, records = [], []
    a0 = alpha_of(level0)
    c0 = count(a0, 1.0, t) if flags & COVERAGE else 0
    for level in levels:
        level = np.asarray(level)
        assert level.dtype == np.float32 and level.ndim == 3 and level.shape[2] == 4
        cur = level.copy()
        if flags & COVERAGE:
            a = cur[..., 3].ravel()
            T = target(c0, a.size, a0.size)
            s, before, after, how = search(a, T, t)
            cur = scale_alpha(cur, s)
            records.append(dict(scale=np.float32(s), target=T, count_before=before, count_after=after))
            if info is not None:
                info.append(how)
        if flags & NORMALIZE:
            cur = normalize(cur, bool(flags & SIGNED_NORMALS))
        out.append(cur)
    return out, records


def box_chain(level0: np.ndarray, levels: int):
    """a plain 2 x 2 box chain for the twin's own tests (float32 levels; odd sizes drop the last row / column)"""
    cur = np.asarray(level0)
    cur = np.stack([alpha_of(cur) if c == 3 else (cur[..., c].astype(np.float64)/255.0).astype(np.float32)
                    if cur.dtype == np.uint8 else cur[..., c].astype(np.float32) for c in range(4)], axis=-1)
    out = []
    for _ in range(1, levels):
        h, w = cur.shape[:2]
        nh, nw = max(1, h >> 1), max(1, w >> 1)
        ys = np.minimum(np.arange(nh)*2, h - 1)
        xs = np.minimum(np.arange(nw)*2, w - 1)
        y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
        c64 = cur.astype(np.float64)
        cur = ((c64[ys][:, xs] + c64[ys][:, x1] + c64[y1][:, xs] + c64[y1][:, x1])/4).astype(np.float32)
        out.append(cur)
    return out
