"""The rate-distortion pass over BC1-5 / BC7 payloads in numpy -- THE DEFINITION of what csrc/rdo.hip computes
(DESIGN.md section 4.14).  It decodes through tests/oracle_lib.py.

The result is the plain payload with byte ranges of some blocks overwritten by the same byte range of an earlier
block of the same segment of their block row:

  * a block row is cut into segments of SEG blocks; a segment is walked left to right, segments are independent;
  * candidate 0 is the block as encoded, candidate 1 + (d - 1) S + s the block with splice s (SPLICES, byte ranges
    [a, b)) taken from the FINAL block at distance d = 1 .. min(L, position in the segment);
  * a candidate the decoder counts as an error block (BC7: the reserved mode, byte 0 == 0) is rejected;
  * SSE: integer, decoded candidate against the source as RGBA8 (quantise()), over the channels the format stores
    AND the mask, texels inside the surface only;
  * rate in bits: 8 BS for candidate 0, 8 (BS - n) + 12 + 2 floor(log2(d BS)) for a splice of n = b - a bytes;
  * the first minimum of J = 16 SSE + round(16 lambda) R over candidate 0 and every candidate whose
    SSE <= SSE(candidate 0) + max_sse_increase wins.

The walk is vectorised over the segments of a surface: step i handles block i of every segment at once."""
import math

import numpy as np

import oracle_lib

L = 16          # lookback, blocks                       (CFRDO_LOOKBACK)
SEG = 64        # blocks of a segment                    (CFRDO_SEG)
NO_CAP = 0xFFFFFFFF

BC1_RGB, BC1_RGBA, BC2, BC3, BC4, BC5, BC7 = 29, 30, 31, 32, 33, 34, 36
UNORM = 0

# (format, type) -> (block bytes, channels stored, splices)                      (kCfrdoRows)
_BC1 = ((0, 8), (0, 4), (4, 8))
TABLE = {
    (BC1_RGB, UNORM): (8, (0, 1, 2), _BC1),
    (BC1_RGBA, UNORM): (8, (0, 1, 2, 3), _BC1),
    (BC2, UNORM): (16, (0, 1, 2, 3), ((0, 16), (8, 16), (8, 12), (12, 16))),
    (BC3, UNORM): (16, (0, 1, 2, 3), ((0, 16), (0, 8), (8, 16), (0, 2), (2, 8), (8, 12), (12, 16))),
    (BC4, UNORM): (8, (0,), ((0, 8), (0, 2), (2, 8))),
    (BC5, UNORM): (16, (0, 1), ((0, 16), (0, 8), (8, 16), (0, 2), (2, 8), (8, 10), (10, 16))),
    (BC7, UNORM): (16, (0, 1, 2, 3), ((0, 16), (8, 16), (0, 8))),
}


def supported(fmt, typ=UNORM) -> bool:
    return (int(fmt), int(typ)) in TABLE


def lambda16(lam) -> int:
    """round(16 lambda), lambda as the float the C ABI carries"""
    lam = float(np.float32(lam))
    if not (0.0 < lam <= 1024.0):
        raise ValueError("lambda outside (0, 1024]")
    return int(math.floor(lam*16.0 + 0.5))


def rate(block_bytes: int, n: int, d: int) -> int:
    return 8*(block_bytes - n) + 12 + 2*((d*block_bytes).bit_length() - 1)


def quantise(src: np.ndarray) -> np.ndarray:
    """The source as RGBA8, floats as the encoders quantise them: round(clamp(f) * 255) in float, NaN -> 0."""
    src = np.asarray(src)
    if src.dtype == np.uint8:
        return src
    f = src.astype(np.float32)
    nan = np.isnan(f)
    f = np.clip(np.where(nan, np.float32(0), f), np.float32(0), np.float32(1))*np.float32(255)
    return np.floor(f.astype(np.float64) + 0.5).astype(np.uint8)


def _decode_blocks(blocks: np.ndarray, fmt, typ) -> np.ndarray:
    """(n, BS) blocks -> (n, 4, 4, 4) RGBA8 texels [block, row, column, channel]"""
    n = blocks.shape[0]
    img = oracle_lib.decode(np.ascontiguousarray(blocks).reshape(-1), fmt, 4*n, 4, typ)
    return img.reshape(4, n, 4, 4).transpose(1, 0, 2, 3)


def rdo(payload, src, fmt, typ=UNORM, lam=1.0, max_sse_increase=None, mask=(True, True, True, True), seg=None):
    """-> (the optimised payload, dict of the six statistics).  src: (h, w, 4) uint8 / float16 / float32.
    seg: segment length for measurements (None: SEG; 0: whole rows)."""
    bs, stored, splices = TABLE[(int(fmt), int(typ))]
    seg = SEG if seg is None else seg
    lam16 = lambda16(lam)
    cap = NO_CAP if max_sse_increase is None else int(max_sse_increase)
    chans = [c for c in stored if mask[c]]
    q = quantise(src)
    h, w = q.shape[:2]
    bx, by = (w + 3)//4, (h + 3)//4
    if seg == 0:
        seg = bx
    nsx = (bx + seg - 1)//seg
    pb = nsx*seg                                            # block row padded to whole segments
    orig = np.zeros((by, pb, bs), np.uint8)
    orig[:, :bx] = np.asarray(payload, np.uint8).reshape(by, bx, bs)
    tex = np.zeros((by*4, pb*4, 4), np.int64)
    inside = np.zeros((by*4, pb*4), bool)
    tex[:h, :w] = q
    inside[:h, :w] = True
    # [segment, block, ...]
    orig = orig.reshape(by*nsx, seg, bs)
    tex = tex.reshape(by, 4, nsx, seg, 4, 4).transpose(0, 2, 3, 1, 4, 5).reshape(by*nsx, seg, 4, 4, 4)
    inside = inside.reshape(by, 4, nsx, seg, 4).transpose(0, 2, 3, 1, 4).reshape(by*nsx, seg, 4, 4)
    length = np.tile(np.minimum(seg, bx - seg*np.arange(nsx)), by)          # blocks of each segment
    final = orig.copy()
    S = len(splices)
    st = dict(blocks=bx*by, blocks_changed=0, sse_before=0, sse_after=0, bits_before=bx*by*8*bs, bits_after=0)
    for i in range(seg):
        act = np.nonzero(length > i)[0]
        if not act.size:
            break
        nd = min(i, L)
        nc = 1 + nd*S
        cands = np.repeat(orig[act, i][:, None, :], nc, axis=1)              # (segments, candidates, BS)
        rates = np.empty(nc, np.int64)
        rates[0] = 8*bs
        for d in range(1, nd + 1):
            for s, (a, b) in enumerate(splices):
                c = 1 + (d - 1)*S + s
                cands[:, c, a:b] = final[act, i - d, a:b]
                rates[c] = rate(bs, b - a, d)
        dec = _decode_blocks(cands.reshape(-1, bs), fmt, typ).reshape(act.size, nc, 4, 4, 4).astype(np.int64)
        diff = (dec - tex[act, i][:, None])[..., chans]
        diff = diff*inside[act, i][:, None, :, :, None]
        sse = (diff*diff).sum(axis=(2, 3, 4))
        ok = sse <= sse[:, :1] + cap if cap != NO_CAP else np.ones_like(sse, bool)
        if int(fmt) == BC7:
            ok &= cands[:, :, 0] != 0                                        # the reserved mode: an error block
        ok[:, 0] = True
        J = np.where(ok, 16*sse + lam16*rates[None, :], np.iinfo(np.int64).max)
        win = np.argmin(J, axis=1)                                           # the first minimum
        rows = np.arange(act.size)
        final[act, i] = cands[rows, win]
        st["blocks_changed"] += int((final[act, i] != orig[act, i]).any(axis=1).sum())
        st["sse_before"] += int(sse[:, 0].sum())
        st["sse_after"] += int(sse[rows, win].sum())
        st["bits_after"] += int(rates[win].sum())
    out = final.reshape(by, pb, bs)[:, :bx].reshape(-1).copy()
    return out, st
