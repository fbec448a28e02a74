"""numpy restatement of the PVRTC1 4 bpp codec of csrc/pvrtc.hip: the decoder and every encoder pass, in the same
order and with the same integer arithmetic, so that the GPU payload is byte-identical to encode() here.

The format (Imagination's published PVRTC1 decompression, the PowerVR SDK's PVRTDecompress; the Khronos Data Format
Specification's PVRTC section): 8-byte blocks of a 32-bit modulation word (2 bits per texel, texel (x, y) at bit
2*(4y + x)) and a 32-bit colour word (bit 0 mode, bits 1-15 colour A, bits 16-31 colour B, bit 15 / bit 31 opaque
flags).  Every texel blends the colours of the four blocks whose centres (texel 4b + 2) surround it, with
wrap-around; blocks are stored in twiddled order.  Arrays are (h, w, 4) uint8, row 0 at the top.

The encoder: load -> init -> modulation -> refine sweeps -> pack.
"""
import numpy as np

RGB, RGBA = 59, 60
LEVEL_SWEEPS = None   # filled below: quality -> list of sweep flags
SW_MODE, SW_CAND, SW_OPAC = 1, 2, 4
RIDGE = 64            # pull of the least-squares solve towards the current colour (keeps it non-singular)
MOD_W = np.array([[0, 3, 5, 8], [0, 4, 4, 8]], np.int64)   # modulation weight by (mode, 2-bit value)
PHASES = ((0, 0), (1, 0), (0, 1), (1, 1))
# quality ladder: every level runs the sweeps of the level below first, then more (SSE is monotone over levels)
LEVEL_SWEEPS = {0: [], 1: [0], 2: [0, SW_MODE], 3: [0, SW_MODE, SW_CAND | SW_MODE, SW_CAND | SW_MODE],
                4: [0, SW_MODE, SW_CAND | SW_MODE, SW_CAND | SW_MODE] + [SW_CAND | SW_MODE | SW_OPAC] * 4}


def is_pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def grid(w, h):
    """(blocks across, blocks down): never fewer than 2 x 2"""
    return max(w // 4, 2), max(h // 4, 2)


def payload_size(w, h):
    bx, by = grid(w, h)
    return bx * by * 8


def twiddle(x, y, bx, by):
    """storage index of block (x, y) in a bx x by grid: Morton order, y in the lower bit of each pair; the longer
    dimension's remaining high bits follow"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    lx, ly = bx.bit_length() - 1, by.bit_length() - 1
    m = min(lx, ly)
    idx = np.zeros(np.broadcast(x, y).shape, np.int64)
    for i in range(m):
        idx |= ((y >> i) & 1) << (2 * i)
        idx |= ((x >> i) & 1) << (2 * i + 1)
    if lx > m:
        idx |= (x >> m) << (2 * m)
    elif ly > m:
        idx |= (y >> m) << (2 * m)
    return idx


def unpack(c):
    """colour word(s) -> (A, B): (..., 4) int64 each; RGB on the 5-bit scale, alpha on the 4-bit scale"""
    c = np.asarray(c).astype(np.int64) & 0xFFFFFFFF
    ao, bo = (c >> 15) & 1, (c >> 31) & 1
    A = np.stack([np.where(ao, (c >> 10) & 31, (c & 0xf00) >> 7 | (c & 0xf00) >> 11),
                  np.where(ao, (c >> 5) & 31, (c & 0xf0) >> 3 | (c & 0xf0) >> 7),
                  np.where(ao, (c & 0x1e) | (c & 0x1e) >> 4, (c & 0xe) << 1 | (c & 0xe) >> 2),
                  np.where(ao, 15, (c & 0x7000) >> 11)], -1)
    B = np.stack([np.where(bo, (c >> 26) & 31, (c & 0xf000000) >> 23 | (c & 0xf000000) >> 27),
                  np.where(bo, (c >> 21) & 31, (c & 0xf00000) >> 19 | (c & 0xf00000) >> 23),
                  np.where(bo, (c >> 16) & 31, (c & 0xf0000) >> 15 | (c & 0xf0000) >> 19),
                  np.where(bo, 15, (c & 0x70000000) >> 27)], -1)
    return A, B


def to8(s):
    """bilinear sums (weights total 16) -> 8 bits: RGB (s >> 6) + (s >> 1), alpha (s >> 4) + s"""
    out = (s >> 6) + (s >> 1)
    out[..., 3] = (s[..., 3] >> 4) + s[..., 3]
    return out


def texel_blocks(px, py, bx, by):
    """the four blocks of texels (px, py) and their bilinear weights: lists of (x, y, weight), P Q R S"""
    u, v = (px + 2) & 3, (py + 2) & 3
    x0 = ((px - 2) >> 2) % bx
    y0 = ((py - 2) >> 2) % by
    x1, y1 = (x0 + 1) % bx, (y0 + 1) % by
    return [(x0, y0, (4 - u) * (4 - v)), (x1, y0, u * (4 - v)), (x0, y1, (4 - u) * v), (x1, y1, u * v)]


def interp_sums(A, B, blocks):
    """per-texel weighted sums of the A and B colours of the four blocks (..., 4)"""
    sa = sum(w[..., None] * A[y, x] for x, y, w in blocks)
    sb = sum(w[..., None] * B[y, x] for x, y, w in blocks)
    return sa, sb


def blend(A8, B8, mode, m, fmt):
    """decoded texel from 8-bit A and B, the block mode and the 2-bit modulation value"""
    w = MOD_W[mode, m][..., None]
    out = (A8 * (8 - w) + B8 * w) >> 3
    if fmt == RGB:
        out[..., 3] = 255
    else:
        out[..., 3] = np.where((mode == 1) & (m == 2), 0, out[..., 3])
    return out


# ---- decoder ------------------------------------------------------------------------------------------------

def split_payload(payload, w, h):
    """payload bytes -> (colour words, modulation words), each (by, bx) uint32 in raster order"""
    bx, by = grid(w, h)
    q = np.frombuffer(np.ascontiguousarray(payload, np.uint8).tobytes()[:bx * by * 8], "<u8")
    ys, xs = np.mgrid[0:by, 0:bx]
    blk = q[twiddle(xs, ys, bx, by)]
    return (blk >> np.uint64(32)).astype(np.uint32), (blk & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def decode(payload, w, h, fmt=RGBA):
    """PVRTC1 4 bpp payload -> (h, w, 4) uint8"""
    assert is_pow2(w) and is_pow2(h)
    bx, by = grid(w, h)
    words, mods = split_payload(payload, w, h)
    A, B = unpack(words)
    py, px = np.mgrid[0:h, 0:w]
    sa, sb = interp_sums(A, B, texel_blocks(px, py, bx, by))
    own_w = words[py >> 2, px >> 2].astype(np.int64)
    own_m = (mods[py >> 2, px >> 2].astype(np.int64) >> (2 * (4 * (py & 3) + (px & 3)))) & 3
    return blend(to8(sa), to8(sb), own_w & 1, own_m, fmt).astype(np.uint8)


def sse(payload, ref, fmt=RGBA):
    """exact per-channel sum of squared differences of the decoded payload against an RGBA8 reference"""
    h, w = ref.shape[:2]
    d = decode(payload, w, h, fmt).astype(np.int64) - ref.astype(np.int64)
    return [int(v) for v in (d * d).sum(axis=(0, 1))]


# ---- encoder ------------------------------------------------------------------------------------------------

def _roundf(v):
    """C roundf of float32 values (half away from zero; v >= 0 here)"""
    f = np.floor(v)
    return f + ((v - f) >= np.float32(0.5))


def to_rgba8(img):
    """the source texels as the kernels read them: uint8 as is; float16 / float32 quantised like toColorBlock,
    (uint8)round(clamp(f, 0, 1) * 255) in float, NaN -> 0"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.int64)
    f = img.astype(np.float32)
    f = np.where(f > 0, f, np.float32(0))            # NaN and negatives -> 0
    f = np.minimum(f, np.float32(1)).astype(np.float32)
    return _roundf((f * np.float32(255)).astype(np.float32)).astype(np.int64)


def expand_source(img):
    """(h, w, 4) source -> the (4 by, 4 bx, 4) texels the encoder fits: surfaces under 8 px repeat themselves"""
    t = to_rgba8(img)
    h, w = t.shape[:2]
    bx, by = grid(w, h)
    ys, xs = np.mgrid[0:4 * by, 0:4 * bx]
    return t[ys % h, xs % w]


def _q5(v):
    return (v * 31 + 127) // 255


def _q4a(v):
    return (v * 15 + 127) // 255


def encode_a(c, opaque):
    """colour A bits (1..15) from RGB on the 5-bit scale and alpha on the 4-bit scale"""
    r, g, b, a = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    op = 0x8000 | r << 10 | g << 5 | ((b * 15 + 15) // 31) << 1
    a3 = np.minimum((a + 1) >> 1, 7)
    tr = a3 << 12 | ((r * 15 + 15) // 31) << 8 | ((g * 15 + 15) // 31) << 4 | ((b * 7 + 15) // 31) << 1
    return np.where(opaque, op, tr)


def encode_b(c, opaque):
    r, g, b, a = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    op = 0x80000000 | r << 26 | g << 21 | b << 16
    a3 = np.minimum((a + 1) >> 1, 7)
    tr = a3 << 28 | ((r * 15 + 15) // 31) << 24 | ((g * 15 + 15) // 31) << 20 | ((b * 15 + 15) // 31) << 16
    return np.where(opaque, op, tr)


def init_words(tex, fmt):
    """A = the per-channel minimum of each block's 16 texels, B the maximum; opaque unless the alpha rounds below
    15 on the 4-bit scale (always opaque for the RGB format); mode 0"""
    H, W = tex.shape[:2]
    blk = tex.reshape(H // 4, 4, W // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(H // 4, W // 4, 16, 4)
    lo, hi = blk.min(axis=2), blk.max(axis=2)
    ca = np.concatenate([_q5(lo[..., :3]), _q4a(lo[..., 3:])], -1)
    cb = np.concatenate([_q5(hi[..., :3]), _q4a(hi[..., 3:])], -1)
    if fmt == RGB:
        return (encode_a(ca, True) | encode_b(cb, True)).astype(np.int64)
    return (encode_a(ca, ca[..., 3] == 15) | encode_b(cb, cb[..., 3] == 15)).astype(np.int64)


def best_mod(A8, B8, t, mode, wch, fmt):
    """exact argmin (first minimum) of the channel-weighted squared error over the four modulation values"""
    best_e = best_m = None
    for m in range(4):
        mm = np.full(mode.shape, m, np.int64)
        d = blend(A8, B8, mode, mm, fmt) - t
        e = (d * d * wch).sum(-1)
        if best_e is None:
            best_e, best_m = e, mm
        else:
            better = e < best_e
            best_e, best_m = np.where(better, e, best_e), np.where(better, mm, best_m)
    return best_m, best_e


def modulation_pass(tex, words, wch, fmt):
    """every texel's modulation value; RGBA blocks also pick their mode here (punch-through only if it lowers the
    block's error)"""
    H, W = tex.shape[:2]
    bx, by = W // 4, H // 4
    A, B = unpack(words)
    py, px = np.mgrid[0:H, 0:W]
    sa, sb = interp_sums(A, B, texel_blocks(px, py, bx, by))
    A8, B8 = to8(sa), to8(sb)
    m0, e0 = best_mod(A8, B8, tex, np.zeros((H, W), np.int64), wch, fmt)
    words = words & ~1
    if fmt == RGB:
        return words, m0
    m1, e1 = best_mod(A8, B8, tex, np.ones((H, W), np.int64), wch, fmt)
    s0 = e0.reshape(by, 4, bx, 4).sum(axis=(1, 3))
    s1 = e1.reshape(by, 4, bx, 4).sum(axis=(1, 3))
    pt = s1 < s0
    words = words | pt.astype(np.int64)
    ptt = pt[py >> 2, px >> 2]
    return words, np.where(ptt, m1, m0)


def _rdiv(n, d):
    """round(n / d) for d > 0, halves up: floor((2n + d) / 2d)"""
    return (2 * n + d) // (2 * d)


# fields of a colour a +-1 candidate may step: (shift, bits) per (colour, opaque)
FIELDS = {(0, 1): [(10, 5), (5, 5), (1, 4)], (0, 0): [(12, 3), (8, 4), (4, 4), (1, 3)],
          (1, 1): [(26, 5), (21, 5), (16, 5)], (1, 0): [(28, 3), (24, 4), (20, 4), (16, 4)]}


def _step_field(word, k):
    """candidate k (0..15) of the +-1 set: colour k >> 3, field (k >> 1) & 3, direction k & 1 (0 down, 1 up);
    the base word where the field does not exist or would leave its range"""
    col, j, up = k >> 3, (k >> 1) & 3, k & 1
    opaque = (word >> (15 if col == 0 else 31)) & 1
    out = word.copy()
    for op in (0, 1):
        fl = FIELDS[(col, op)]
        if j >= len(fl):
            continue
        sh, bits = fl[j]
        v = (word >> sh) & ((1 << bits) - 1)
        nv = v + (1 if up else -1)
        ok = (opaque == op) & (nv >= 0) & (nv < (1 << bits))
        out = np.where(ok, (word & ~(((1 << bits) - 1) << sh)) | (nv << sh), out)
    return out


def refine_phase(tex, words, mods, wch, fmt, ox, oy, flags):
    """one parity phase: every block (ox + 2i, oy + 2j) refits A and B over the 7x7 texels it influences"""
    H, W = tex.shape[:2]
    bx, by = W // 4, H // 4
    cy, cx = np.mgrid[oy:by:2, ox:bx:2]
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    n = cx.size
    dj, di = np.mgrid[0:7, 0:7]
    di, dj = di.reshape(-1), dj.reshape(-1)
    px = (4 * cx[:, None] - 1 + di[None, :]) % W            # (n, 49)
    py = (4 * cy[:, None] - 1 + dj[None, :]) % H
    hw = np.array([1, 2, 3, 4, 3, 2, 1], np.int64)
    wP = hw[di][None, :] * hw[dj][None, :]
    wP = np.broadcast_to(wP, px.shape)
    t = tex[py, px]
    A, B = unpack(words)
    sa, sb = interp_sums(A, B, texel_blocks(px, py, bx, by))
    Ac, Bc = A[cy, cx], B[cy, cx]                            # (n, 4): the centre's current colours
    ra = sa - wP[..., None] * Ac[:, None, :]                 # the neighbours' part of the sums
    rb = sb - wP[..., None] * Bc[:, None, :]
    own = (di >= 1) & (di <= 4) & (dj >= 1) & (dj <= 4)      # texel lies in the centre block
    nb_mode = words[py >> 2, px >> 2] & 1
    m_cur = mods[py, px].astype(np.int64)
    # the region's error as it stands
    d = blend(to8(sa), to8(sb), nb_mode, m_cur, fmt) - t
    old = (d * d * wch).sum(-1).sum(-1)
    # least squares for the centre's A and B, the current modulation held
    w = MOD_W[nb_mode, m_cur]
    al, be = (8 - w) * wP, w * wP
    pt = (nb_mode == 1) & (m_cur == 2)                       # punch-through zero: its alpha ignores A and B
    ala, bea = np.where(pt, 0, al), np.where(pt, 0, be)
    cur = np.concatenate([Ac[:, None, :], Bc[:, None, :]], 1)  # (n, 2, 4)
    sol = np.zeros((n, 2, 4), np.int64)
    for ch in range(4):
        a_, b_ = (al, be) if ch < 3 else (ala, bea)
        fn, fd = (255, 31) if ch < 3 else (17, 1)
        c = (8 - w) * ra[..., ch] + w * rb[..., ch]
        y = t[..., ch] * 128 * fd - fn * c
        saa = (a_ * a_).sum(-1) + RIDGE
        sbb = (b_ * b_).sum(-1) + RIDGE
        sab = (a_ * b_).sum(-1)
        say = (a_ * y).sum(-1) + RIDGE * fn * cur[:, 0, ch]
        sby = (b_ * y).sum(-1) + RIDGE * fn * cur[:, 1, ch]
        det = saa * sbb - sab * sab
        na = sbb * say - sab * sby
        nbv = saa * sby - sab * say
        top = 31 if ch < 3 else 15
        sol[:, 0, ch] = np.clip(_rdiv(na, fn * det), 0, top)
        sol[:, 1, ch] = np.clip(_rdiv(nbv, fn * det), 0, top)
    mode_c = words[cy, cx] & 1
    if fmt == RGB:
        flags &= ~(SW_MODE | SW_OPAC)
        opa = opb = np.ones(n, bool)
    else:
        opa, opb = sol[:, 0, 3] == 15, sol[:, 1, 3] == 15
    base = encode_a(sol[:, 0], opa) | encode_b(sol[:, 1], opb) | mode_c
    cands = [base]
    if flags & SW_CAND:
        cands += [_step_field(base, k) for k in range(16)]
    if flags & SW_MODE:
        cands.append(base ^ 1)
    if flags & SW_OPAC:
        cands += [encode_a(sol[:, 0], ~opa) | encode_b(sol[:, 1], opb) | mode_c,
                  encode_a(sol[:, 0], opa) | encode_b(sol[:, 1], ~opb) | mode_c,
                  encode_a(sol[:, 0], ~opa) | encode_b(sol[:, 1], ~opb) | mode_c]

    def evaluate(cw):
        ca, cb = unpack(cw)
        a8 = to8(ra + wP[..., None] * ca[:, None, :])
        b8 = to8(rb + wP[..., None] * cb[:, None, :])
        mode = np.where(own[None, :], (cw & 1)[:, None], nb_mode)
        return best_mod(a8, b8, t, mode, wch, fmt)

    best_s = best_w = None
    for cw in cands:
        s = evaluate(cw)[1].sum(-1)
        if best_s is None:
            best_s, best_w = s, cw
        else:
            better = s < best_s
            best_s, best_w = np.where(better, s, best_s), np.where(better, cw, best_w)
    keep = best_s <= old
    m_new = evaluate(best_w)[0]
    words = words.copy()
    mods = mods.copy()
    words[cy[keep], cx[keep]] = best_w[keep]
    mods[py[keep], px[keep]] = m_new[keep]
    return words, mods


def total_sse(tex, words, mods, wch, fmt):
    H, W = tex.shape[:2]
    A, B = unpack(words)
    py, px = np.mgrid[0:H, 0:W]
    sa, sb = interp_sums(A, B, texel_blocks(px, py, W // 4, H // 4))
    d = blend(to8(sa), to8(sb), words[py >> 2, px >> 2] & 1, mods.astype(np.int64), fmt) - tex
    return int((d * d * wch).sum())


def pack(words, mods):
    """colour words and per-texel modulation -> payload bytes in twiddled order"""
    by, bx = words.shape
    m = mods.astype(np.uint64).reshape(by, 4, bx, 4).transpose(0, 2, 1, 3).reshape(by, bx, 16)
    mw = (m << (2 * np.arange(16, dtype=np.uint64))).sum(-1).astype(np.uint64)
    blk = mw | (words.astype(np.uint64) & np.uint64(0xFFFFFFFF)) << np.uint64(32)
    out = np.zeros(bx * by, np.uint64)
    ys, xs = np.mgrid[0:by, 0:bx]
    out[twiddle(xs, ys, bx, by)] = blk
    return np.frombuffer(out.astype("<u8").tobytes(), np.uint8).copy()


def weights(fmt, mask=(1, 1, 1, 1)):
    w = np.array([1 if m else 0 for m in mask], np.int64)
    if fmt == RGB:
        w[3] = 0
    return w


def encode(img, fmt=RGBA, quality=2, mask=(1, 1, 1, 1), trace=None):
    """(h, w, 4) uint8 / float16 / float32 source, both sides powers of two -> payload bytes.  trace: a list that
    receives the total weighted SSE after the modulation pass and after every sweep"""
    h, w = np.asarray(img).shape[:2]
    assert is_pow2(w) and is_pow2(h) and fmt in (RGB, RGBA)
    tex = expand_source(img)
    wch = weights(fmt, mask)
    words = init_words(tex, fmt)
    words, mods = modulation_pass(tex, words, wch, fmt)
    if trace is not None:
        trace.append(total_sse(tex, words, mods, wch, fmt))
    for flags in LEVEL_SWEEPS[quality]:
        for ox, oy in PHASES:
            words, mods = refine_phase(tex, words, mods, wch, fmt, ox, oy, flags)
        if trace is not None:
            trace.append(total_sse(tex, words, mods, wch, fmt))
    return pack(words, mods)
