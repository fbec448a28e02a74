"""ASTC beyond the photograph: sources that make the rarely winning parts of the encoder's subset win (four and three
partitions painted from the format's own partition hash, grey content for the luminance endpoint modes, fixed chroma
times a luminance for base + scale, void extents), a parser of one 16-byte block written from the specification, the
law that ties the parser to the independent decoder, and the census conditions both the oracle's and the kernel's
payloads are held to.  CPU only: nothing here imports the GPU library.

tests/test_astc_cases.py holds all of it for the oracle alone; tests/test_gpu_astc_modes.py compares the kernel."""
import collections
import ctypes
import functools

import numpy as np

import oracle_lib as O
from cuttlefish_amd import synth

FOOT = {43: (4, 4), 44: (5, 4), 45: (5, 5), 46: (6, 5), 47: (6, 6), 48: (8, 5), 49: (8, 6), 50: (8, 8), 51: (10, 5),
        52: (10, 6), 53: (10, 8), 54: (10, 10), 55: (12, 10), 56: (12, 12)}
FORMATS = sorted(FOOT)
# the five footprints of the grey / scaled / void-extent parity runs and the three of the metric variants
FIVE = [43, 44, 47, 51, 56]
METRIC_FORMATS = [43, 47, 51]
HDR_FORMATS = [43, 47, 54]
BLOCKS_X, BLOCKS_Y = 10, 6
NORMAL, HIGH, HIGHEST = 2, 3, 4
UFLOAT = 4

# (levels, bits, trits, quints) of the weight and the colour ranges (specification, "Integer Sequence Encoding")
WQ = [(2, 1, 0, 0), (3, 0, 1, 0), (4, 2, 0, 0), (5, 0, 0, 1), (6, 1, 1, 0), (8, 3, 0, 0), (10, 1, 0, 1), (12, 2, 1, 0),
      (16, 4, 0, 0), (20, 2, 0, 1), (24, 3, 1, 0), (32, 5, 0, 0)]
CQ = [(6, 1, 1, 0), (8, 3, 0, 0), (10, 1, 0, 1), (12, 2, 1, 0), (16, 4, 0, 0), (20, 2, 0, 1), (24, 3, 1, 0), (32, 5, 0, 0),
      (40, 3, 0, 1), (48, 4, 1, 0), (64, 6, 0, 0), (80, 4, 0, 1), (96, 5, 1, 0), (128, 7, 0, 0), (160, 5, 0, 1),
      (192, 6, 1, 0), (256, 8, 0, 0)]
WLEVELS = [q[0] for q in WQ]
HDR_CEMS = (2, 3, 7, 11, 14, 15)
# what the oracle reaches on the HDR painted sources on at least three blocks per footprint (measured; the rest is
# named in tests/test_astc_cases.py::test_hdr_census_of_the_oracle)
HDR_ALPHAS = {"one": 0, "ldr": 2, "hdr": 1}
HDR_REACHED_PARTS = (1, 2, 3, 4)
HDR_REACHED_CEMS = (7, 11, 14, 15)


def ise_bits(count, q):
    return count*q[1] + ((8*count + 4)//5 if q[2] else 0) + ((7*count + 2)//3 if q[3] else 0)


# ---- the partition hash (specification, "Partition Pattern Generation") ---------------------------------------

def _hash52(p):
    m = 0xFFFFFFFF
    p ^= p >> 15
    p = (p - (p << 17)) & m
    p = (p + (p << 7)) & m
    p = (p + (p << 4)) & m
    p ^= p >> 5
    p = (p + (p << 16)) & m
    p ^= p >> 7
    p ^= p >> 3
    p ^= (p << 6) & m
    p ^= p >> 17
    return p


@functools.lru_cache(maxsize=None)
def select_partition(seed, bw, bh, parts):
    """(bh, bw) array: the partition of every texel of a 2-D block under a 10-bit seed; the "small block" form (the
    coordinates doubled) below 31 texels"""
    y, x = np.mgrid[0:bh, 0:bw]
    if bw*bh < 31:
        x, y = x << 1, y << 1
    seed += (parts - 1)*1024
    r = _hash52(seed)
    s = [r & 15, (r >> 4) & 15, (r >> 8) & 15, (r >> 12) & 15, (r >> 16) & 15, (r >> 20) & 15, (r >> 24) & 15,
         (r >> 28) & 15]
    s = [v*v for v in s]
    if seed & 1:
        sh1, sh2 = (4 if seed & 2 else 5), (6 if parts == 3 else 5)
    else:
        sh1, sh2 = (6 if parts == 3 else 5), (4 if seed & 2 else 5)
    s = [v >> (sh1 if i % 2 == 0 else sh2) for i, v in enumerate(s)]
    a = (s[0]*x + s[1]*y + (r >> 14)) & 63
    b = (s[2]*x + s[3]*y + (r >> 10)) & 63
    c = (s[4]*x + s[5]*y + (r >> 6)) & 63 if parts >= 3 else np.zeros_like(x)
    d = (s[6]*x + s[7]*y + (r >> 2)) & 63 if parts >= 4 else np.zeros_like(x)
    out = np.where((a >= b) & (a >= c) & (a >= d), 0, np.where((b >= c) & (b >= d), 1, np.where(c >= d, 2, 3)))
    out.setflags(write=False)
    return out


# ---- sources ---------------------------------------------------------------------------------------------------

COLOURS = np.array([[230, 40, 30], [30, 200, 60], [40, 50, 230], [240, 225, 40]], np.int64)
# (not evenly spaced: four evenly spaced grey levels ARE the four weight levels of one partition, and where the
# footprint's full-resolution grid of two-bit weights fits -- 6x5, 8x5 -- that block wins everywhere)
GREYS = np.array([5, 100, 130, 250], np.int64)
ALPHAS = np.array([255, 40, 140, 200], np.int64)
KINDS = ("colour", "grey", "alpha")
# seeds of the painted sources that are not 0, (format, partitions, kind): chosen so that the ORACLE's payload holds the
# floors of check_census (three-partition blocks with alpha at 4x4 Highest, 8x5 and 10x5 Normal; four-partition grey
# blocks at 8x5, 8x6 and 10x5, where seed 0 gives 5, 1 and 5)
PAINT_SEEDS = {(43, 3, "alpha"): 11, (48, 3, "alpha"): 1, (51, 3, "alpha"): 6,
               (48, 4, "grey"): 1, (49, 4, "grey"): 3, (51, 4, "grey"): 1}


def _painted_seeds(rng, bw, bh, parts, count):
    """per block a seed under which all `parts` partitions occur with at least two texels each"""
    seeds = []
    while len(seeds) < count:
        s = int(rng.integers(0, 1024))
        n = np.bincount(select_partition(s, bw, bh, parts).reshape(-1), minlength=parts)
        if (n >= 2).all():
            seeds.append(s)
    return seeds


@functools.lru_cache(maxsize=None)
def painted(bw, bh, parts, kind, seed=0, blocks=(BLOCKS_X, BLOCKS_Y)):
    """blocks painted from the partition hash: every partition one of four far-apart colours (grey levels; colours
    with an alpha of their own), +-3 noise"""
    assert kind in KINDS
    rng = np.random.default_rng([seed, bw, bh, parts, KINDS.index(kind)])
    nx, ny = blocks
    img = np.zeros((ny*bh, nx*bw, 4), np.int64)
    for i, s in enumerate(_painted_seeds(rng, bw, bh, parts, nx*ny)):
        part = select_partition(s, bw, bh, parts)
        order = rng.permutation(4)
        tile = img[(i//nx)*bh:(i//nx + 1)*bh, (i % nx)*bw:(i % nx + 1)*bw]
        if kind == "grey":
            tile[..., :3] = GREYS[order][part][..., None]
        else:
            tile[..., :3] = COLOURS[order][part]
        tile[..., 3] = ALPHAS[order][part] if kind == "alpha" else 255
    noise = rng.integers(-3, 4, img.shape)
    if kind == "grey":
        noise[..., :3] = noise[..., :1]
    if kind != "alpha":
        noise[..., 3] = 0
    out = np.clip(img + noise, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grey(bw, bh, alpha):
    """the photograph with R = G = B = the channel mean; opaque, or with the photograph's alpha band"""
    img = synth.photo(BLOCKS_X*bw, BLOCKS_Y*bh, seed=700 + bw*16 + bh, alpha=alpha)
    g = ((img[..., :3].astype(np.int64).sum(-1) + 1)//3).astype(np.uint8)
    img[..., 0] = img[..., 1] = img[..., 2] = g
    img.setflags(write=False)
    return img


CHROMA = np.array([[1.0, 0.55, 0.2], [0.3, 1.0, 0.6], [0.45, 0.25, 1.0], [1.0, 0.9, 0.35]])
# the photograph's seed where it is not 800 + 16 bw + bh (10x6: two base + scale blocks at Normal under that one)
SCALED_SEEDS = {(10, 6): 801}


@functools.lru_cache(maxsize=None)
def scaled(bw, bh, alpha):
    """a fixed chroma per quarter of the image times the photograph's luminance: the content of base + scale; the
    bottom block row carries one channel of its own (the content of a second plane), a different one per quarter"""
    img = synth.photo(BLOCKS_X*bw, BLOCKS_Y*bh, seed=SCALED_SEEDS.get((bw, bh), 800 + bw*16 + bh), alpha=alpha)
    other =synth.photo(BLOCKS_X*bw, BLOCKS_Y*bh, seed=900 + bw*16 + bh, alpha=True)
    lum = img[..., :3].astype(np.float64).mean(-1)
    h, w = lum.shape
    out = img.copy()
    q = w//4 + 1
    for k in range(4):
        xs = slice(k*q, min((k + 1)*q, w))
        out[:, xs, :3] = np.clip(np.floor(lum[:, xs, None]*CHROMA[k] + 0.5), 0, 255).astype(np.uint8)
        plane = other[-2*bh:, xs].astype(np.int64)
        if k < 3:
            out[-2*bh:, xs, k] = ((plane[..., 0] + plane[..., 1] + plane[..., 2])//3).astype(np.uint8)
        elif alpha:
            out[-2*bh:, xs, 3] = ((plane[..., 0] + plane[..., 1] + plane[..., 2])//3).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ramps(bw, bh):
    """smooth blocks: per block a plane (every third one bent) per channel, full to faint contrast -- the content of
    coarse weight grids with many weight levels"""
    rng = np.random.default_rng([5, bw, bh])
    y, x = np.mgrid[0:bh, 0:bw]
    u, v = x/(bw - 1.0), y/(bh - 1.0)
    img = np.zeros((BLOCKS_Y*bh, BLOCKS_X*bw, 4), np.float64)
    for i in range(BLOCKS_X*BLOCKS_Y):
        tile = img[(i//BLOCKS_X)*bh:(i//BLOCKS_X + 1)*bh, (i % BLOCKS_X)*bw:(i % BLOCKS_X + 1)*bw]
        amp = [1.0, 0.5, 0.2, 0.06][i % 4]
        ang = rng.random()*2*np.pi
        t = 0.5 + 0.5*(np.cos(ang)*(u - 0.5) + np.sin(ang)*(v - 0.5))*1.4
        if i % 3 == 0:
            t = t*t
        lo, hi = rng.random(4)*(1 - amp), None
        hi = lo + amp*rng.random(4)
        tile[...] = lo + (hi - lo)*t[..., None]
        if i % 2:
            tile[..., 3] = 1.0
    out = np.clip(np.floor(img*255.0 + 0.5), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


# solid colours of the void-extent source: 0 and 255, bytes, and (for the float form) values between two bytes
_SOLID8 = [(0, 0, 0, 0), (255, 255, 255, 255), (0, 0, 0, 255), (255, 0, 128, 255), (1, 2, 3, 4), (254, 127, 129, 1),
           (77, 77, 77, 77), (18, 52, 86, 120)]
_SOLIDF = [(0.3, 0.5, 0.7, 0.9), (0.001, 0.998, 0.4999, 0.5001), (1.5, -0.25, 0.0019607, 1.0), (0.1, 0.2, 0.6, 0.0)]


def _void_layout(bw, bh, colours, dtype):
    """tiles of one block each: the solid colours; then the same colours with one texel changed (first, last, middle
    texel in turn); the image is cut three texels short on the right and one at the bottom, inside solid blocks whose
    colour so continues into the ragged edge"""
    nx = 6
    tiles = [(c, None) for c in colours] + [(c, i % 3) for i, c in enumerate(colours)]
    while len(tiles) % nx:
        tiles.append((colours[len(tiles) % len(colours)], None))
    ny = len(tiles)//nx + 1
    img = np.zeros((ny*bh, nx*bw, 4), dtype)
    for i, (c, odd) in enumerate(tiles):
        tile = img[(i//nx)*bh:(i//nx + 1)*bh, (i % nx)*bw:(i % nx + 1)*bw]
        tile[...] = np.array(c, dtype)
        if odd is not None:
            y, x = [(0, 0), (bh - 1, bw - 1), (bh//2, bw//2)][odd]
            tile[y, x, 1] = (255 - c[1]) if dtype == np.uint8 else 1.0 - min(max(c[1], 0.0), 1.0)
    img[-bh:] = np.array(colours[3], dtype)                       # a solid bottom row of blocks ...
    for i in range(nx):                                            # ... of a colour per block
        img[-bh:, i*bw:(i + 1)*bw] = np.array(colours[i % len(colours)], dtype)
    return np.ascontiguousarray(img[:-1, :-3])


@functools.lru_cache(maxsize=None)
def void_extent_u8(bw, bh):
    out = _void_layout(bw, bh, _SOLID8, np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def void_extent_f32(bw, bh):
    """the bytes of void_extent_u8 as u8 / 255 would not show a loader that keeps more than eight bits: float values
    between two bytes, above 1, below 0 and next to a rounding tie"""
    out = _void_layout(bw, bh, [tuple(v/255.0 for v in c) for c in _SOLID8[:4]] + _SOLIDF, np.float32)
    out.setflags(write=False)
    return out


def as_float(img, dtype=np.float32):
    """u8 / 255 as the loader's float source"""
    return np.ascontiguousarray((img.astype(np.float64)/255.0).astype(dtype))


@functools.lru_cache(maxsize=None)
def hdr_painted(bw, bh, parts, alpha, seed=0):
    """the painted source as float32 under the HDR profiles: the four colours at exposures 2^-4 .. 2^8, one exposure
    per partition, +-3 % noise; alpha "one", "ldr" (0..1 per partition) or "hdr" (an exposure of its own)"""
    rng = np.random.default_rng([seed, bw, bh, parts, 77])
    nx, ny = BLOCKS_X, BLOCKS_Y
    img = np.ones((ny*bh, nx*bw, 4), np.float64)
    for i, s in enumerate(_painted_seeds(rng, bw, bh, parts, nx*ny)):
        part = select_partition(s, bw, bh, parts)
        order = rng.permutation(4)
        expo = np.exp2(rng.integers(-4, 9, 4).astype(np.float64))
        tile = img[(i//nx)*bh:(i//nx + 1)*bh, (i % nx)*bw:(i % nx + 1)*bw]
        tile[..., :3] = (COLOURS[order]/255.0*expo[:, None])[part]
        if alpha == "ldr":
            tile[..., 3] = (ALPHAS[order]/255.0)[part]
        elif alpha == "hdr":
            tile[..., 3] = np.exp2(rng.integers(-4, 9, 4).astype(np.float64))[part]
    noise = 1.0 + 0.03*(rng.random(img.shape)*2 - 1)
    if alpha == "one":
        noise[..., 3] = 1.0
    out = np.ascontiguousarray((img*noise).astype(np.float32))
    out.setflags(write=False)
    return out


# ---- one block, parsed -----------------------------------------------------------------------------------------

def block_mode(mode):
    """(N, M, weight range index, dual) of an 11-bit block mode; None for reserved ones and void extent
    (specification, "Block Mode")"""
    R0, A, B = (mode >> 4) & 1, (mode >> 5) & 3, (mode >> 7) & 3
    H, D = (mode >> 9) & 1, (mode >> 10) & 1
    if mode & 3:
        R1, R2 = mode & 1, (mode >> 1) & 1
        k = (mode >> 2) & 3
        if k == 0: N, M = B + 4, A + 2
        elif k == 1: N, M = B + 8, A + 2
        elif k == 2: N, M = A + 2, B + 8
        elif not (mode >> 8) & 1: N, M = A + 2, (B & 1) + 6
        else: N, M = (B & 1) + 2, A + 2
    else:
        if not mode & 0xC:
            return None
        R1, R2 = (mode >> 2) & 1, (mode >> 3) & 1
        if B == 0: N, M = 12, A + 2
        elif B == 1: N, M = A + 2, 12
        elif B == 2: N, M, H, D = A + 6, ((mode >> 9) & 3) + 6, 0, 0
        elif A == 0: N, M = 6, 10
        elif A == 1: N, M = 10, 6
        else: return None
    r = (R2 << 2) | (R1 << 1) | R0
    if r < 2:
        return None
    return N, M, (r - 2) + 6*H, D


def _trits(T):
    if (T >> 2) & 7 == 7:
        C = ((T >> 5) << 2) | (T & 3)
        t4 = t3 = 2
    else:
        C = T & 31
        if (T >> 5) & 3 == 3:
            t4, t3 = 2, T >> 7
        else:
            t4, t3 = T >> 7, (T >> 5) & 3
    if C & 3 == 3:
        t2, t1, t0 = 2, C >> 4, (((C >> 3) & 1) << 1) | (((C >> 2) & 1) & ~((C >> 3) & 1))
    elif (C >> 2) & 3 == 3:
        t2, t1, t0 = 2, 2, C & 3
    else:
        t2, t1, t0 = C >> 4, (C >> 2) & 3, (((C >> 1) & 1) << 1) | ((C & 1) & ~((C >> 1) & 1))
    return t0, t1, t2, t3, t4


def _quints(Q):
    if (Q >> 1) & 3 == 3 and (Q >> 5) & 3 == 0:
        b0 = Q & 1
        return 4, 4, (b0 << 2) | ((((Q >> 4) & 1) & ~b0) << 1) | (((Q >> 3) & 1) & ~b0)
    if (Q >> 1) & 3 == 3:
        q2, C = 4, (((Q >> 3) & 3) << 3) | ((~(Q >> 5) & 3) << 1) | (Q & 1)
    else:
        q2, C = (Q >> 5) & 3, Q & 31
    if C & 7 == 5:
        q1, q0 = 4, (C >> 3) & 3
    else:
        q1, q0 = (C >> 3) & 3, C & 7
    return q0, q1, q2


def ise_decode(q, v, pos, count):
    """`count` values of range q from bit `pos` of the block (an int, bit 0 first); a value is its trit or quint above
    its plain bits"""
    _, bits, trits, quints = q
    stream = (v >> pos) & ((1 << ise_bits(count, q)) - 1)
    out, p = [], 0

    def take(n):
        nonlocal p
        r = (stream >> p) & ((1 << n) - 1)
        p += n
        return r
    if trits:
        while len(out) < count:
            m, T = [], 0
            for n, sh in ((2, 0), (2, 2), (1, 4), (2, 5), (1, 7)):
                m.append(take(bits))
                T |= take(n) << sh
            out += [(t << bits) | lo for t, lo in zip(_trits(T), m)]
    elif quints:
        while len(out) < count:
            m, Q = [], 0
            for n, sh in ((3, 0), (2, 3), (2, 5)):
                m.append(take(bits))
                Q |= take(n) << sh
            out += [(t << bits) | lo for t, lo in zip(_quints(Q), m)]
    else:
        out = [take(bits) for _ in range(count)]
    return out[:count]


def unquant_colour(q, val):
    """specification, "Endpoint Unquantization": bit replication, or T = D*C + B, T ^= A"""
    _, bits, trits, quints = q
    if not trits and not quints:
        r, sh = 0, 8 - bits
        while sh > -bits:
            r |= (val << sh) if sh >= 0 else (val >> -sh)
            sh -= bits
        return r & 255
    m, D = val & ((1 << bits) - 1), val >> bits
    A = 0x1FF if m & 1 else 0
    x = m >> 1
    if trits:
        B, C = [(0, 204), (x*0x116, 93), ((x << 7) | (x << 2) | x, 44), ((x << 6) | x, 22), ((x << 5) | (x >> 2), 11),
                ((x << 4) | (x >> 4), 5)][bits - 1]
    else:
        B, C = [(0, 113), (x*0x10C, 54), ((x << 7) | (x << 1) | (x >> 1), 26), ((x << 6) | (x >> 1), 13),
                ((x << 5) | (x >> 3), 6)][bits - 1]
    T = (D*C + B) ^ A
    return (A & 0x80) | (T >> 2)


Block = collections.namedtuple("Block", "void hdr_void colour parts seed cems dual ccs grid wlevels clevels values "
                               "contracted")


def _transfer(a, b):
    """bit_transfer_signed of the specification"""
    b = (b >> 1) | (a & 0x80)
    a = (a >> 1) & 0x3F
    return (a - 0x40 if a & 0x20 else a), b


def _contracted(cem, v):
    """whether the decoder applies blue contraction to this value list (modes 8 / 12 and 9 / 13), else None"""
    if cem in (8, 12):
        return v[1] + v[3] + v[5] < v[0] + v[2] + v[4]
    if cem in (9, 13):
        return sum(_transfer(v[2*i + 1], v[2*i])[0] for i in range(3)) < 0
    return None


def parse_block(blk, bw, bh):
    """-> Block, or None for a block the specification calls illegal.  For void extent only `colour` (four 16-bit
    values) and `hdr_void` are set.  `clevels` is the colour range the bits left over allow; `values` holds the
    unquantised endpoint values of each partition, `contracted` the blue-contraction flag of each."""
    v = int.from_bytes(bytes(bytearray(blk)), "little")
    mode = v & 0x7FF
    if (mode & 0x1FF) == 0x1FC:
        if (v >> 10) & 3 != 3:
            return None
        return Block(True, bool((mode >> 9) & 1), tuple((v >> (64 + 16*c)) & 0xFFFF for c in range(4)), 0, 0, (), 0,
                     None, None, 0, 0, (), ())
    bm = block_mode(mode)
    if bm is None:
        return None
    N, M, wq, dual = bm
    nw = N*M*(2 if dual else 1)
    wbits = ise_bits(nw, WQ[wq])
    parts = ((v >> 11) & 3) + 1
    if N > bw or M > bh or nw > 64 or not 24 <= wbits <= 96 or (dual and parts == 4):
        return None
    extra = 0
    if parts == 1:
        cems, seed, cstart = [(v >> 13) & 15], 0, 17
    else:
        seed, sel, cstart = (v >> 13) & 1023, (v >> 23) & 63, 29
        if sel & 3 == 0:
            cems = [sel >> 2]*parts
        else:
            extra = 3*parts - 4
            sel |= ((v >> (128 - wbits - extra)) & ((1 << extra) - 1)) << 6
            base = (sel & 3) - 1
            cems = [((base + ((sel >> (2 + p)) & 1)) << 2) | ((sel >> (2 + parts + 2*p)) & 3) for p in range(parts)]
    nvals = sum(2*((c >> 2) + 1) for c in cems)
    cbits = 128 - wbits - cstart - extra - (2 if dual else 0)
    if nvals > 18 or cbits < (13*nvals + 4)//5:
        return None
    level = max(i for i, q in enumerate(CQ) if ise_bits(nvals, q) <= cbits)
    ccs = (v >> (128 - wbits - extra - 2)) & 3 if dual else None
    raw = ise_decode(CQ[level], v, cstart, nvals)
    vals, values, pos = [unquant_colour(CQ[level], r) for r in raw], [], 0
    for c in cems:
        k = 2*((c >> 2) + 1)
        values.append(tuple(vals[pos:pos + k]))
        pos += k
    return Block(False, False, None, parts, seed, tuple(cems), dual, ccs, (N, M), WLEVELS[wq], CQ[level][0],
                 tuple(values), tuple(_contracted(c, x) for c, x in zip(cems, values)))


def parse_payload(payload, fmt):
    bw, bh = FOOT[int(fmt)]
    return [parse_block(b, bw, bh) for b in np.asarray(payload, np.uint8).reshape(-1, 16)]


def describe(blocks, fmt):
    """the parsed fields of blocks, for a failure message"""
    out = []
    for b in parse_payload(blocks, fmt):
        if b is None:
            out.append("illegal")
        elif b.void:
            out.append("void extent %s" % (b.colour,))
        else:
            out.append("P%d seed %d cem %s%s grid %dx%d w%d c%d values %s%s" % (
                b.parts, b.seed, list(b.cems), " dual ccs %d" % b.ccs if b.dual else "", b.grid[0], b.grid[1], b.wlevels,
                b.clevels, list(b.values), " contracted" if any(b.contracted) else ""))
    return out


# ---- the law between the parser and the independent decoder -----------------------------------------------------

def unpack_endpoints(cem, values):
    """the endpoint pair the oracle's decoder (pinned to Mesa's) reads from a value list"""
    L = O.lib()
    L.cfo_astc_unpack_endpoints.restype = ctypes.c_int
    v = (ctypes.c_int*8)(*(list(values) + [0]*(8 - len(values))))
    e0, e1 = (ctypes.c_int*4)(), (ctypes.c_int*4)()
    kind = L.cfo_astc_unpack_endpoints(int(cem), v, e0, e1)
    return kind, np.array(e0[:]), np.array(e1[:])


def check_endpoint_law(payload, fmt, width, height):
    """Every channel of every texel the decoder returns lies between the two endpoint values of the texel's partition,
    as the PARSER read them: LDR interpolation is convex on the 16-bit expansions e*257 and its top byte is monotone,
    so the margin is zero.  A wrong seed, CEM position, ISE read, unquantisation or contraction flag breaks it.
    -> number of blocks checked"""
    bw, bh = FOOT[int(fmt)]
    dec, bad = O.decode_astc(payload, int(fmt), width, height)
    assert bad == 0
    bx = (width + bw - 1)//bw
    checked = 0
    for i, b in enumerate(parse_payload(payload, fmt)):
        assert b is not None, "block %d is illegal" % i
        tile = dec[(i//bx)*bh:(i//bx + 1)*bh, (i % bx)*bw:(i % bx + 1)*bw].astype(np.int64)
        if b.void:
            assert (tile == np.array(b.colour) >> 8).all(), (i, b.colour)
            continue
        part = select_partition(b.seed, bw, bh, b.parts)[:tile.shape[0], :tile.shape[1]]
        lo, hi = np.zeros((b.parts, 4), np.int64), np.zeros((b.parts, 4), np.int64)
        for p in range(b.parts):
            kind, e0, e1 = unpack_endpoints(b.cems[p], b.values[p])
            assert kind == 0, (i, b.cems)
            lo[p], hi[p] = np.minimum(e0, e1), np.maximum(e0, e1)
        inside = (tile >= lo[part]) & (tile <= hi[part])
        assert inside.all(), "block %d (%s): a texel outside its partition's endpoints" % (
            i, describe(np.asarray(payload).reshape(-1, 16)[i], fmt)[0])
        checked += 1
    return checked


# ---- the census ------------------------------------------------------------------------------------------------

def census(payload, fmt):
    """what a payload holds, as counters over its blocks: 'parts', 'cem' (of the first partition: the encoder gives
    all partitions of a block one mode), 'cem_multi' (the same over multi-partition blocks), 'ccs' (plane selector of
    dual-plane blocks), 'wlevels', 'clevels', 'contracted' ((cem, flag) of modes 8 / 12 / 9 / 13), 'void', 'illegal'"""
    c = {k: collections.Counter() for k in ("parts", "cem", "cem_multi", "ccs", "wlevels", "clevels", "contracted")}
    c["void"] = c["illegal"] = 0
    for b in parse_payload(payload, fmt):
        if b is None:
            c["illegal"] += 1
        elif b.void:
            c["void"] += 1
        else:
            c["parts"][b.parts] += 1
            c["cem"][b.cems[0]] += 1
            if b.parts > 1:
                c["cem_multi"][b.cems[0]] += 1
            if b.dual:
                c["ccs"][b.ccs] += 1
            c["wlevels"][b.wlevels] += 1
            c["clevels"][b.clevels] += 1
            for cem, flag in zip(b.cems, b.contracted):
                if flag is not None:
                    c["contracted"][(cem, bool(flag))] += 1
    return c


def census_line(c):
    def cnt(k):
        return " ".join("%s:%d" % kv for kv in sorted(c[k].items(), key=lambda kv: str(kv[0])))
    return "P{%s} cem{%s} ccs{%s} w{%s} c{%s} void %d" % (cnt("parts"), cnt("cem"), cnt("ccs"), cnt("wlevels"),
                                                        cnt("clevels"), c["void"])


# Floors of the census, per source key.  A source key is a tuple: ("painted", P, kind), ("grey", alpha),
# ("scaled", alpha), ("void", "u8" | "f32"), ("ramps",), ("hdr_painted", P, alpha).  The floors hold from Normal up:
# the levels below search too little for them (Lowest takes one partition only).
FOUR_PARTITION_FLOOR = 4
THREE_PARTITION_FLOOR = 4
MODE_FLOOR = 3
# painted alpha at 4x4: no three-partition block wins at Normal (three partitions with alpha are mode 10, 18 values)
THREE_PARTITION_ALPHA_HIGHEST_ONLY = (43,)


def source(key, fmt):
    bw, bh = FOOT[int(fmt)]
    if key[0] == "painted":
        return painted(bw, bh, key[1], key[2], PAINT_SEEDS.get((int(fmt), key[1], key[2]), 0))
    if key[0] == "grey":
        return grey(bw, bh, key[1])
    if key[0] == "scaled":
        return scaled(bw, bh, key[1])
    if key[0] == "void":
        return void_extent_u8(bw, bh) if key[1] == "u8" else void_extent_f32(bw, bh)
    if key[0] == "ramps":
        return ramps(bw, bh)
    if key[0] == "hdr_painted":
        return hdr_painted(bw, bh, key[1], key[2])
    raise KeyError(key)


PAINTED4 = [("painted", 4, k) for k in KINDS]
PAINTED3 = [("painted", 3, k) for k in KINDS]
PLAIN = [("grey", False), ("grey", True), ("scaled", False), ("scaled", True), ("void", "u8"), ("void", "f32"), ("ramps",)]


def levels_of(key):
    """the levels a source is encoded at: those at which its feature is searched"""
    if key[0] == "painted":
        return (HIGHEST,) if key[1] == 4 else (NORMAL, HIGH, HIGHEST)
    return (0, 1, NORMAL, HIGH, HIGHEST)


@functools.lru_cache(maxsize=None)
def ref(key, fmt, quality, typ=0, alpha=1, color_space=0, mask=(1, 1, 1, 1)):
    """the oracle's payload of a source, encoded once per session"""
    out = O.encode(source(key, fmt), int(fmt), typ=typ, quality=quality, threads=16, alpha=alpha,
                   color_space=color_space, mask=mask)
    out.setflags(write=False)
    return out


def unorm8(img):
    """the loader's bytes of a float source: clamp, times 255, round half up (in float32)"""
    if img.dtype == np.uint8:
        return img
    f = np.clip(np.nan_to_num(img.astype(np.float32), nan=0.0), np.float32(0), np.float32(1))*np.float32(255)
    return np.floor(f.astype(np.float64) + 0.5).astype(np.uint8)


def solid_blocks(img, fmt):
    """which blocks of an image are one colour after the loader (edge texels replicated): bool per block, row-major"""
    bw, bh = FOOT[int(fmt)]
    u = unorm8(img)
    h, w = u.shape[:2]
    by, bx = (h + bh - 1)//bh, (w + bw - 1)//bw
    u = np.pad(u, ((0, by*bh - h), (0, bx*bw - w), (0, 0)), mode="edge")
    t = u.reshape(by, bh, bx, bw, 4).transpose(0, 2, 1, 3, 4).reshape(by*bx, bh*bw, 4)
    return (t == t[:, :1]).all(axis=(1, 2)), t[:, 0]


def check_census(key, fmt, quality, payload):
    """the conditions a payload of source `key` at `fmt` / `quality` has to meet, whoever encoded it -> its census"""
    fmt = int(fmt)
    c = census(payload, fmt)
    what = "%s %dx%d level %d: %s" % (key, FOOT[fmt][0], FOOT[fmt][1], quality, census_line(c))
    assert c["illegal"] == 0, what
    if key[0] == "void":
        # exactly the solid blocks are void extents, and each holds its colour as byte * 257
        solid, colour = solid_blocks(source(key, fmt), fmt)
        blocks = parse_payload(payload, fmt)
        assert [b.void for b in blocks] == list(solid), what
        for b, s, col in zip(blocks, solid, colour):
            assert not s or (not b.hdr_void and b.colour == tuple(int(v)*257 for v in col)), (what, b.colour, col)
        assert solid.sum() >= 12 and (~solid).sum() >= 6, what
    if quality < NORMAL:
        return c
    if key[0] == "painted":
        _, parts, kind = key
        if parts == 4 and kind in ("colour", "grey") and quality == HIGHEST:
            assert c["parts"][4] >= FOUR_PARTITION_FLOOR, what
        if parts == 4 and kind == "grey" and quality == HIGHEST:
            assert c["cem_multi"][0] >= FOUR_PARTITION_FLOOR, what          # ... and they are luminance blocks
        if parts == 3 and quality in (NORMAL, HIGHEST):
            if kind != "alpha" or quality == HIGHEST or fmt not in THREE_PARTITION_ALPHA_HIGHEST_ONLY:
                assert c["parts"][3] >= THREE_PARTITION_FLOOR, what
                if kind == "alpha":
                    assert c["cem_multi"][10] >= THREE_PARTITION_FLOOR, what
    elif key[0] == "grey":
        assert c["cem"][0] >= MODE_FLOOR, what
        if key[1]:
            assert c["cem"][4] >= MODE_FLOOR, what
    elif key[0] == "scaled":
        assert c["cem"][10 if key[1] else 6] >= MODE_FLOOR, what
    return c


def legal_weight_levels(bw, bh):
    """the weight ranges some legal grid of the footprint can carry (24..96 weight bits, at most 64 weights), single
    or dual plane"""
    out = set()
    for mode in range(2048):
        bm = block_mode(mode)
        if bm is None or (mode & 0x1FF) == 0x1FC:
            continue
        N, M, wq, dual = bm
        nw = N*M*(2 if dual else 1)
        if N <= bw and M <= bh and nw <= 64 and 24 <= ise_bits(nw, WQ[wq]) <= 96:
            out.add(WLEVELS[wq])
    return out


# ---- launch shapes ---------------------------------------------------------------------------------------------

SHAPE_FORMATS = [43, 47, 50, 56]
SHAPE_LEVELS = [NORMAL, HIGH]


def launch_shape(lib, fmt, quality, hdr, bx):
    """(waves per workgroup, 168-register build, blocks a wave searches at a time) of a surface with bx blocks per
    row, from the library's own plan (no device needed)"""
    bw, bh = FOOT[int(fmt)]
    shape = (ctypes.c_uint32*4)()
    lib.cfhip_debug_astc_launch_shape.restype = ctypes.c_int
    lib.cfhip_debug_astc_launch_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.c_uint32*4]
    assert lib.cfhip_debug_astc_launch_shape(bw, bh, quality, 1 if hdr else 0, bx, shape) == 0
    return int(shape[0]), bool(shape[1]), int(shape[2])


SWEEP_ALWAYS = (1, 2, 3, 57)


@functools.lru_cache(maxsize=None)
def sweep_image(bw, bh, hdr):
    """100 x 3 blocks painted with three partitions, the bottom row a texel short; under the HDR profiles as float32,
    every block column at an exposure of its own (2^-4 .. 2^8)"""
    img = painted(bw, bh, 3, "colour", seed=9, blocks=(100, 3))[:-1]
    if hdr:
        expo = np.exp2((np.arange(img.shape[1])//bw*5) % 13 - 4.0)
        f = (img.astype(np.float64)/255.0)**2.2
        f[..., :3] *= expo[None, :, None]
        img = f.astype(np.float32)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


def sweep_widths(lib, fmt, quality, hdr):
    """How SWEEP below was made.  For every shape the plan yields for 1..100 blocks per row: the first width that
    fills the shape's last workgroup, and the width that leaves the FEWEST blocks in a last workgroup after a full one
    (a single block where the plan keeps the shape for it: it weighs the idle share of a row's last workgroup, so most
    shapes are never chosen for such a width); 1, 2, 3 and one width above 48.
    -> ({shape: (full, ragged)}, sorted widths)"""
    shapes = {}
    for bx in range(1, 101):
        shapes.setdefault(launch_shape(lib, fmt, quality, hdr, bx), []).append(bx)
    picks = {}
    for shape, widths in shapes.items():
        per = shape[0]*4
        full = [b for b in widths if b % per == 0]
        over = sorted((b % per, b) for b in widths if b % per and b > per)
        picks[shape] = (full[0] if full else None, over[0][1] if over else None)
    widths = set(SWEEP_ALWAYS)
    for full, over in picks.values():
        widths |= {b for b in (full, over) if b}
    return picks, sorted(widths)


# (footprint, level, HDR) -> (the shapes the plan yields for 1..100 blocks per row, assuming 160 KB of LDS per
# compute unit; the blocks per row of the sweep).  Made by sweep_widths(); tests/test_astc_cases.py derives both again
# from the library's plan and holds this table to them.
SWEEP = {
    (43, 2, False): ([(4, True, 2), (5, True, 2), (6, True, 2), (7, True, 2)],
                     [1, 2, 3, 16, 20, 24, 28, 33, 49, 57, 65, 85]),
    (43, 3, False): ([(4, True, 1), (5, True, 1), (6, True, 1), (7, True, 1), (9, True, 1), (11, True, 1)],
                     [1, 2, 3, 16, 20, 24, 28, 36, 37, 44, 49, 57, 65, 73, 85]),
    (47, 2, False): ([(4, False, 2), (9, True, 2)],
                     [1, 2, 3, 16, 17, 36, 57, 65]),
    (47, 3, False): ([(4, False, 1), (9, True, 1), (10, True, 1), (11, True, 1)],
                     [1, 2, 3, 16, 17, 36, 40, 44, 57, 65, 73, 81]),
    (50, 2, False): ([(4, False, 2), (5, False, 2), (6, False, 2), (7, False, 2), (8, False, 2)],
                     [1, 2, 3, 16, 20, 24, 28, 32, 33, 41, 57, 85, 97]),
    (50, 3, False): ([(4, False, 1), (9, True, 1), (10, True, 1)],
                     [1, 2, 3, 16, 17, 36, 40, 57, 65, 73]),
    (56, 2, False): ([(4, False, 2), (5, False, 2), (6, False, 2)],
                     [1, 2, 3, 16, 20, 24, 25, 49, 57, 81]),
    (56, 3, False): ([(4, False, 1), (5, False, 1), (6, False, 1), (7, False, 1), (8, False, 1)],
                     [1, 2, 3, 16, 20, 24, 28, 32, 33, 41, 57, 85, 97]),
    (43, 2, True): ([(4, False, 2), (5, False, 2), (6, False, 2)],
                    [1, 2, 3, 16, 20, 24, 49, 57, 65, 81]),
    (43, 3, True): ([(4, False, 1), (5, False, 1), (6, False, 1), (7, False, 1)],
                    [1, 2, 3, 16, 20, 24, 28, 33, 49, 57, 65, 85]),
    (47, 2, True): ([(4, False, 2), (5, False, 2), (6, False, 2), (7, False, 2), (8, False, 2)],
                    [1, 2, 3, 16, 20, 24, 28, 32, 33, 41, 57, 85, 97]),
    (47, 3, True): ([(4, False, 1), (5, False, 1), (6, False, 1), (7, False, 1), (8, False, 1)],
                    [1, 2, 3, 16, 20, 24, 28, 32, 33, 41, 57, 85, 97]),
    (50, 2, True): ([(4, False, 2), (5, False, 2), (6, False, 2)],
                    [1, 2, 3, 16, 20, 24, 25, 49, 57, 81]),
    (50, 3, True): ([(4, False, 1), (5, False, 1), (6, False, 1), (7, False, 1)],
                    [1, 2, 3, 16, 20, 24, 28, 29, 33, 57, 61, 97]),
    (56, 2, True): ([(4, False, 2)],
                    [1, 2, 3, 16, 17, 57]),
    (56, 3, True): ([(4, False, 1), (5, False, 1)],
                    [1, 2, 3, 16, 20, 49, 57, 65]),
}
