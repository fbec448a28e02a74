"""The rate-distortion pass with copies from the block row above, in numpy -- THE DEFINITION of what
cfhip_rdo2d_kernel (csrc/rdo.hip) computes.  It follows everything tests/rdo_ref.py says
and adds:

  * a surface is cut into tiles of SEG blocks x TILE_ROWS block rows, counted from its top-left corner; tiles are
    independent; inside a tile rows go top to bottom and the blocks of a row left to right;
  * a surface has up-candidates iff row_above and (bx + UP/2) BS <= window_bytes (bx: blocks of a row), that is, iff
    every block the pass may copy from above lies inside the compressor's window; otherwise its result is
    rdo_ref.rdo's, bytes and statistics;
  * for the block at position i of its segment, not in the first row of its tile, candidate
    1 + L S + u S + s is the block with splice s taken from the FINAL block at position i + dx, dx = u - UP/2,
    u = 0 .. UP - 1, of the row above in the same tile; it exists iff 0 <= i + dx < blocks of the segment;
  * its rate is 8 (BS - n) + 12 + 2 floor(log2((bx - dx) BS)): the match lies (bx - dx) BS bytes back;
  * the horizontal candidates keep their numbers 1 .. L S, and the first minimum of J wins as before.

The walk is vectorised over the tiles of a surface: a step handles block i of row r of every tile at once."""
import numpy as np

import rdo_ref
from rdo_ref import L, NO_CAP, SEG, TABLE, UNORM

TILE_ROWS = 8   # block rows of a tile                                   (CFRDO_TILE_ROWS)
UP = 8          # positions of the row above: dx = -UP/2 .. UP/2 - 1     (CFRDO_UP)
WINDOW = 32768  # deflate's                                              (window_bytes == 0)


def rate_up(block_bytes: int, n: int, bx: int, dx: int) -> int:
    return 8*(block_bytes - n) + 12 + 2*(((bx - dx)*block_bytes).bit_length() - 1)


def has_up(bx: int, block_bytes: int, row_above, window_bytes=WINDOW, up=UP) -> bool:
    return bool(row_above) and (bx + up//2)*block_bytes <= window_bytes


def rdo2d(payload, src, fmt, typ=UNORM, lam=1.0, max_sse_increase=None, mask=(True, True, True, True),
          row_above=False, window_bytes=WINDOW, tile_rows=TILE_ROWS, seg=None, up=UP):
    """-> (the optimised payload, dict of the six statistics), as rdo_ref.rdo.  tile_rows, seg (None: SEG; 0: whole
    rows) and up are there for measurements."""
    bs, stored, splices = TABLE[(int(fmt), int(typ))]
    q = rdo_ref.quantise(src)
    h, w = q.shape[:2]
    bx, by = (w + 3)//4, (h + 3)//4
    if not has_up(bx, bs, row_above, window_bytes, up):
        return rdo_ref.rdo(payload, src, fmt, typ, lam, max_sse_increase, mask, seg)
    seg = SEG if seg is None else seg
    lam16 = rdo_ref.lambda16(lam)
    cap = NO_CAP if max_sse_increase is None else int(max_sse_increase)
    chans = [c for c in stored if mask[c]]
    if seg == 0:
        seg = bx
    R = tile_rows
    nsx, nty = (bx + seg - 1)//seg, (by + R - 1)//R
    pb, pby = nsx*seg, nty*R                                 # the surface padded to whole tiles
    orig = np.zeros((pby, pb, bs), np.uint8)
    orig[:by, :bx] = np.asarray(payload, np.uint8).reshape(by, bx, bs)
    tex = np.zeros((pby*4, pb*4, 4), np.int64)
    inside = np.zeros((pby*4, pb*4), bool)
    tex[:h, :w] = q
    inside[:h, :w] = True
    # [tile, row, block, ...]
    orig = orig.reshape(nty, R, nsx, seg, bs).transpose(0, 2, 1, 3, 4).reshape(nty*nsx, R, seg, bs)
    tex = tex.reshape(nty, R, 4, nsx, seg, 4, 4).transpose(0, 3, 1, 4, 2, 5, 6).reshape(nty*nsx, R, seg, 4, 4, 4)
    inside = inside.reshape(nty, R, 4, nsx, seg, 4).transpose(0, 3, 1, 4, 2, 5).reshape(nty*nsx, R, seg, 4, 4)
    length = np.tile(np.minimum(seg, bx - seg*np.arange(nsx)), nty)              # blocks of a row of each tile
    rows = np.repeat(np.minimum(R, by - R*np.arange(nty)), nsx)                  # rows of each tile
    final = orig.copy()
    S = len(splices)
    nc = 1 + (L + up)*S
    # per candidate: its rate, whether it copies from the row above, its distance to the left or its dx, its bytes
    rates = np.empty(nc, np.int64)
    above = np.zeros(nc, bool)
    dist, dxs = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
    taken = np.zeros((nc, bs), bool)
    rates[0] = 8*bs
    for s, (a, b) in enumerate(splices):
        for d in range(1, L + 1):
            c = 1 + (d - 1)*S + s
            rates[c], dist[c] = rdo_ref.rate(bs, b - a, d), d
            taken[c, a:b] = True
        for u in range(up):
            c, dx = 1 + (L + u)*S + s, u - up//2
            # a position right of the surface's last block never exists: any rate will do there
            rates[c], above[c], dxs[c] = (rate_up(bs, b - a, bx, dx) if bx > dx else 0), True, dx
            taken[c, a:b] = True
    st = dict(blocks=bx*by, blocks_changed=0, sse_before=0, sse_after=0, bits_before=bx*by*8*bs, bits_after=0)
    for r in range(R):
        for i in range(seg):
            act = np.nonzero((rows > r) & (length > i))[0]
            if not act.size:
                break
            pos = np.where(above, i + dxs, i - dist)                             # where each candidate copies from
            exists = np.where(above, r > 0, True) & (pos >= 0)
            exists = exists[None, :] & (pos[None, :] < length[act][:, None])     # (tiles, candidates)
            there = final[act[:, None], np.where(above, max(r - 1, 0), r)[None, :], np.clip(pos, 0, seg - 1)[None, :]]
            cands = np.where(taken[None] & exists[:, :, None], there, orig[act, r, i][:, None, :])
            dec = rdo_ref._decode_blocks(cands.reshape(-1, bs), fmt, typ).reshape(act.size, nc, 4, 4, 4).astype(np.int64)
            diff = (dec - tex[act, r, i][:, None])[..., chans]
            diff = diff*inside[act, r, i][:, None, :, :, None]
            sse = (diff*diff).sum(axis=(2, 3, 4))
            ok = exists & (sse <= sse[:, :1] + cap if cap != NO_CAP else True)
            if int(fmt) == rdo_ref.BC7:
                ok &= cands[:, :, 0] != 0                                        # the reserved mode: an error block
            ok[:, 0] = True
            J = np.where(ok, 16*sse + lam16*rates[None, :], np.iinfo(np.int64).max)
            win = np.argmin(J, axis=1)                                           # the first minimum
            k = np.arange(act.size)
            final[act, r, i] = cands[k, win]
            st["blocks_changed"] += int((final[act, r, i] != orig[act, r, i]).any(axis=1).sum())
            st["sse_before"] += int(sse[:, 0].sum())
            st["sse_after"] += int(sse[k, win].sum())
            st["bits_after"] += int(rates[win].sum())
    out = final.reshape(nty, nsx, R, seg, bs).transpose(0, 2, 1, 3, 4).reshape(pby, pb, bs)[:by, :bx].reshape(-1).copy()
    return out, st
