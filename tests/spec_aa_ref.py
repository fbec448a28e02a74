"""The numpy twin of specular anti-aliasing (cfhip_spec_aa_array_device): every step of the
definition in include/cuttlefish_hip.h in float64 / int64, in the order written.  The kernels must return its bits.

numpy evaluates each operation on its own (no contraction), rint rounds ties to even, int64 -> float64 rounds to
nearest even and sqrt is IEEE: the same functions the device applies.
"""
import numpy as np

PERCEPTUAL, SIGNED_NORMALS, RECONSTRUCT_Z = 1, 2, 4
FIELDS = ("clamped", "saturated", "max_added", "reserved")
Q30, Q32 = 1073741824.0, 4294967296.0
MAX_SIDE, MAX_TEXELS = 32768, 1 << 30


def decode(image: np.ndarray) -> np.ndarray:
    """(h, w, c) uint8 / float16 / float32 -> float64: RGBA8 (double)((float)(v / 255.0)), the others widened"""
    if image.dtype == np.uint8:
        return (image.astype(np.float64)/255.0).astype(np.float32).astype(np.float64)
    if image.dtype not in (np.float16, np.float32):
        raise TypeError(image.dtype)
    return image.astype(np.float64)


def level_dims(width: int, height: int, k: int):
    return max(1, width >> k), max(1, height >> k)


def chain_levels(width: int, height: int) -> int:
    return int(max(width, height)).bit_length()


def quantise_normals(normals: np.ndarray, flags: int):
    """(h, w, 4) storage -> (qx, qy, qz) int64, unit normals in Q30; a degenerate normal is +z"""
    c = decode(normals)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    with np.errstate(all="ignore"):
        if not flags & SIGNED_NORMALS:
            x, y, z = x*2.0 - 1.0, y*2.0 - 1.0, z*2.0 - 1.0
        if flags & RECONSTRUCT_Z:
            z = np.sqrt(np.fmax(0.0, 1.0 - (x*x + y*y)))
        length = np.sqrt((x*x + y*y) + z*z)
        ok = np.isfinite(length) & (length > 0.0)
        safe = np.where(ok, length, 1.0)
        nx = np.where(ok, x/safe, 0.0)
        ny = np.where(ok, y/safe, 0.0)
        nz = np.where(ok, z/safe, 1.0)
    return tuple(np.rint(n*Q30).astype(np.int64) for n in (nx, ny, nz))


def quantise_roughness(r: np.ndarray, flags: int) -> np.ndarray:
    """decoded roughness (float64) -> qa int64, alpha^2 in Q32"""
    r = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        r = np.where(r >= 0.0, r, 0.0)
        r = np.where(r > 1.0, 1.0, r)
    alpha = r*r if flags & PERCEPTUAL else r
    return np.rint(alpha*alpha*Q32).astype(np.int64)


def footprint_edges(size0: int, k: int):
    """the first level-0 column (or row) of every texel of level k; the last texel runs to size0"""
    return np.arange(max(1, size0 >> k), dtype=np.int64) << k


def footprint_counts(size0: int, k: int) -> np.ndarray:
    e = footprint_edges(size0, k)
    return np.diff(np.append(e, size0))


def direct_sums(q: np.ndarray, k: int) -> np.ndarray:
    """(h, w) int64 level-0 values -> their sums over the footprints of level k"""
    h, w = q.shape
    rows = np.add.reduceat(q, footprint_edges(h, k), axis=0)
    return np.add.reduceat(rows, footprint_edges(w, k), axis=1)


def child_sums(prev: np.ndarray) -> np.ndarray:
    """the sums of level k from those of level k - 1: children 2x and 2x + 1, and 2x + 2 at an odd end"""
    h, w = prev.shape
    rows = np.add.reduceat(prev, np.arange(max(1, h >> 1))*2, axis=0)
    return np.add.reduceat(rows, np.arange(max(1, w >> 1))*2, axis=1)


def finish_a2(sx, sy, sz, sa, n, variance_scale: float, max_variance: float):
    """moments and texel counts of one level -> (a2 in float64 before it is stored, the clamped texels, the saturated
    ones, what was added)"""
    scale, maxv = np.float64(np.float32(variance_scale)), np.float64(np.float32(max_variance))
    dn = n.astype(np.float64)
    d30, d32 = dn*Q30, dn*Q32
    mx, my, mz = sx.astype(np.float64)/d30, sy.astype(np.float64)/d30, sz.astype(np.float64)/d30
    a2m = sa.astype(np.float64)/d32
    l2 = (mx*mx + my*my) + mz*mz
    below, positive = l2 < 1.0, l2 > 0.0
    lobe = below & positive
    with np.errstate(all="ignore"):
        safe = np.where(lobe, l2, 0.5)
        length = np.sqrt(safe)
        t = (1.0 - safe)/(length*(3.0 - safe))
    clamped = (below & ~positive) | (lobe & ~(t < maxv))
    v = np.where(lobe & (t < maxv), t, np.where(clamped, maxv, 0.0))
    added = scale*v
    total = a2m + added
    saturated = ~(total < 1.0)
    return np.where(saturated, 1.0, total), clamped, saturated, added


def finish(sx, sy, sz, sa, n, flags: int, variance_scale: float, max_variance: float):
    """moments and texel counts of one level -> (its stored values as float32, its record as a dict)"""
    a2, clamped, saturated, added = finish_a2(sx, sy, sz, sa, n, variance_scale, max_variance)
    r = np.sqrt(a2)
    if flags & PERCEPTUAL:
        r = np.sqrt(r)
    record = dict(clamped=int(clamped.sum()), saturated=int(saturated.sum()),
                  max_added=int(added.astype(np.float32).view(np.uint32).max()), reserved=0)
    return r.astype(np.float32), record


def moments(normals: np.ndarray, roughness0, channel: int, flags: int):
    """level 0 quantised: (qx, qy, qz, qa).  roughness0: an (h, w, 4) image or the roughness of every texel"""
    qx, qy, qz = quantise_normals(normals, flags)
    if isinstance(roughness0, np.ndarray):
        if roughness0.shape[:2] != normals.shape[:2]:
            raise ValueError("the roughness map has the size of the normal map")
        qa = quantise_roughness(decode(roughness0)[..., channel], flags)
    else:
        base = np.float64(np.float32(roughness0))
        qa = np.broadcast_to(quantise_roughness(base, flags), qx.shape).copy()
    return qx, qy, qz, qa


def specular_aa(normals: np.ndarray, roughness0, levels_count: int, channel: int = 1, flags: int = PERCEPTUAL,
                variance_scale: float = 1.0, max_variance: float = 1.0, hierarchical: bool = True):
    """-> (the values of `channel` for levels 1 ... levels_count - 1, float32 (h_k, w_k); their records).
    hierarchical: each level's sums from the level before (as the kernels reduce), else straight from level 0 -- the
    same integers either way."""
    h, w = normals.shape[:2]
    if not 2 <= levels_count <= chain_levels(w, h) or not 0 <= channel <= 3 or w*h > MAX_TEXELS:
        raise ValueError("bad arguments")
    q = moments(normals, roughness0, channel, flags)
    values, records = [], []
    cur = q
    for k in range(1, levels_count):
        cur = tuple(child_sums(s) for s in cur) if hierarchical else tuple(direct_sums(s, k) for s in q)
        n = np.outer(footprint_counts(h, k), footprint_counts(w, k))
        val, rec = finish(*cur, n, flags, variance_scale, max_variance)
        values.append(val)
        records.append(rec)
    return values, records
