"""The numpy twin of cfhip_height_ao_array_device (include/cuttlefish_hip.h): ambient occlusion
of a height field by a horizon scan, every step an IEEE double operation in the order the header writes it.  Vectorised
over the texels; tests/test_height_ao_ref.py holds the plain triple loop it is checked against."""
import math

import numpy as np

WRAP_X, WRAP_Y, UNIFORM, FALLOFF = 1, 2, 4, 8          # cfhip_height_ao_params.flags
FIELDS = ("occluded", "darkest", "reserved0", "reserved1")
MAX_SIDE, MAX_RADIUS = 32768, 64
# the first quadrant of every direction set; the other three are these turned by (x, y) -> (-y, x)
BASES = {8: ((1, 0), (1, 1)),
         16: ((1, 0), (2, 1), (1, 1), (1, 2)),
         32: ((1, 0), (3, 1), (2, 1), (3, 2), (1, 1), (2, 3), (1, 2), (1, 3))}


def in_order_sum(w):
    """S = 0.0; S = S + w_d for d = 0 ... D - 1"""
    S = 0.0
    for x in w:
        S = S + float(x)
    return S


def directions(D):
    """-> (vx, vy, weight): D integer vectors and each one's share of the circle, half the angle between its two
    neighbours over 2 pi, from atan2 of the neighbours' cross and dot products (both exact integers)"""
    vec = []
    for q in range(4):
        for x, y in BASES[D]:
            for _ in range(q):
                x, y = -y, x
            vec.append((x, y))
    w = []
    for d in range(D):
        (ax, ay), (bx, by) = vec[d - 1], vec[(d + 1) % D]
        w.append(0.5*math.atan2(ax*by - ay*bx, ax*bx + ay*by)/(2.0*math.pi))
    # A flat surface must come out as exactly 1: while the sum in direction order misses 1.0, the next base direction
    # (i = 0, 1, ...), in all four quadrants, moves one unit in the last place towards it.  D = 8 and 16 need no step,
    # D = 32 two: the weights stay within an ulp of the angles.
    i = 0
    while in_order_sum(w) != 1.0:
        up = in_order_sum(w) < 1.0
        for q in range(4):
            w[q*(D//4) + i] = math.nextafter(w[q*(D//4) + i], 2.0 if up else 0.0)
        i = (i + 1) % (D//4)
    return (np.array([v[0] for v in vec], np.int32), np.array([v[1] for v in vec], np.int32), np.array(w, np.float64))


def reach(radius, vx, vy):
    """R_d: the largest k with k^2 (vx^2 + vy^2) <= R^2, in integers"""
    n, k = int(vx)*int(vx) + int(vy)*int(vy), 0
    while (k + 1)*(k + 1)*n <= radius*radius:
        k += 1
    return k


def gain(radius, vx, vy, k, falloff):
    """g(d, k)"""
    n = int(vx)*int(vx) + int(vy)*int(vy)
    r = np.float64(1.0)/(np.float64(k)*np.sqrt(np.float64(n)))
    if falloff:
        r = r*(np.float64(1.0) - np.float64(k*k*n)/np.float64((radius + 1)*(radius + 1)))
    return r


def decode(image, channel):
    """h(p) as float32: RGBA8 (float)(v / 255.0), half -> float, float as stored; a non-finite value reads 0"""
    c = np.asarray(image)[..., channel]
    if c.dtype == np.uint8:
        h = (c.astype(np.float64)/255.0).astype(np.float32)
    else:
        h = c.astype(np.float32)
    return np.where(np.isfinite(h), h, np.float32(0.0)).astype(np.float32)


def occlusion(h, radius, height=1.0, D=16, strength=1.0, bias=0.0, flags=0, table=None):
    """h: (rows, cols) float32 heights -> (v as float64, the texels with any t_d > 0 as a bool array)"""
    h = np.asarray(h, np.float32)
    rows, cols = h.shape
    vx, vy, wd = directions(D) if table is None else table
    H = np.float64(np.float32(height))*h.astype(np.float64)
    b, s = np.float64(np.float32(bias)), np.float64(np.float32(strength))
    ys, xs = np.arange(rows), np.arange(cols)
    S = np.zeros(h.shape, np.float64)
    occluded = np.zeros(h.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            m = np.full(h.shape, -np.inf)
            for k in range(1, reach(radius, vx[d], vy[d]) + 1):
                qx, qy = xs + k*int(vx[d]), ys + k*int(vy[d])
                okx = np.ones(cols, bool) if flags & WRAP_X else (qx >= 0) & (qx < cols)
                oky = np.ones(rows, bool) if flags & WRAP_Y else (qy >= 0) & (qy < rows)
                Hq = H[np.ix_(qy % rows, qx % cols)]
                c = (Hq - H)*gain(radius, vx[d], vy[d], k, flags & FALLOFF)
                m = np.where(np.outer(oky, okx), np.maximum(m, c), m)
            t = np.maximum(0.0, m - b)
            occluded |= t > 0.0
            if flags & UNIFORM:
                vis = 1.0 - t/np.sqrt(1.0 + t*t)
            else:
                vis = 1.0/(1.0 + t*t)
            S = S + wd[d]*vis
    return np.minimum(1.0, np.maximum(0.0, 1.0 - s*(1.0 - S))), occluded


def stored(v, dtype):
    """v as a component of the destination's pixel type"""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.floor(v*255.0 + 0.5).astype(np.uint8)
    return v.astype(np.float32).astype(dtype)              # half: nearest-even from the float


def height_ao(src, dst, radius, height=1.0, D=16, channel=0, mask=1, strength=1.0, bias=0.0, flags=0, table=None):
    """src, dst: (rows, cols, 4) images -> (dst with v in the components of the mask, the record as a dict)"""
    v, occ = occlusion(decode(src, channel), radius, height, D, strength, bias, flags, table)
    out = np.array(dst, copy=True)
    q = stored(v, out.dtype)
    for ch in range(4):
        if mask >> ch & 1:
            out[..., ch] = q
    darkest = int(v.astype(np.float32).min().view(np.uint32))
    return out, dict(occluded=int(occ.sum()), darkest=darkest, reserved0=0, reserved1=0)
