"""Shared ETC1 / ETC2 / EAC cases (plain numpy + the CPU oracle; no GPU): block classifiers, the sources whose
payloads reach every colour mode, every EAC table and multiplier, the flat laws, the flat-block bounds and the
float rounding boundaries of the loaders.  Used by tests/test_etc_cases.py (the oracle alone) and
tests/test_gpu_etc_modes.py (the HIP kernels); every law takes the encoder as a callable
encode(img, fmt, typ=0, quality=2, **kw) -> payload bytes.

What the oracle's payloads of these sources hold at each level (the HIP kernels' payloads are byte-equal, so
these are their counts too).  Blocks per class of colour_source() (seed 7, 28 x 16 = 448 blocks, 64 per class
in the source; RGBA8 codes a8_source(), whose colour blocks are the same):

    format    level    indiv f0  indiv f1  diff f0  diff f1    T    H  planar
    ETC1      Lowest        141       160       79       68    0    0       0
    ETC1      Low           150       169       70       59    0    0       0
    ETC1      Normal        142       163       76       67    0    0       0
    ETC1      High          142       166       75       65    0    0       0
    ETC1      Highest       143       163       76       66    0    0       0
    ETC2 RGB  Lowest        113       123       74       67    0    0      71
    ETC2 RGB  Low            84        92       41       35   71   61      64
    ETC2 RGB  Normal         85        85       49       44   61   60      64
    ETC2 RGB  High           84        88       48       42   60   62      64
    ETC2 RGB  Highest        85        86       48       43   60   62      64

RGB8A1 on a1_source() (colour seed 55), opaque blocks / blocks with transparent texels per mode:

    level    differential        T        H   planar
    Lowest       86 / 336   0 /   0   0 /   0  26 /   0
    Low          32 / 117  29 / 208  35 /  11  16 /   0
    Normal       42 / 144  26 / 177  28 /  15  16 /   0
    High         41 / 145  26 / 174  29 /  17  16 /   0
    Highest      41 / 143  26 / 176  29 /  17  16 /   0

EAC: blocks per table 0..15, per multiplier 1..15 and the range of bases, RG11 payload of eac_source(typ) (seeds
1 / 2; 2 x 448 blocks) and the alpha blocks of RGBA8 on a8_source() (seed 5):

    UNorm Lowest  tables  48  46  64  38  32  62  30  48  54  88  56  78  54  42  80  76
                  mults   62  64  66  74  68  66  76  62  60  76  58  44  48  36  36  bases 0..254
    UNorm Low     tables  48  46  64  38  32  62  30  48  54  88  56  78  54  42  80  76
                  mults   62  64  66  74  68  66  76  62  60  76  58  44  48  36  36  bases 0..254
    UNorm Normal  tables  44  52  70  34  28  62  32  44  54  92  56  74  56  42  84  72
                  mults   62  62  64  74  72  68  72  70  54  76  50  50  48  38  36  bases 0..253
    UNorm High    tables  44  46  62  32  36  66  34  48  56  92  58  70  56  42  84  70
                  mults   62  60  64  74  64  76  72  68  56  78  50  50  46  40  36  bases 0..251
    UNorm Highest tables  44  46  62  32  36  66  34  48  56  92  58  70  56  42  84  70
                  mults   62  60  64  74  64  76  72  68  56  78  50  50  46  40  36  bases 0..251
    SNorm Lowest  tables  44  44  90  38  36  46  18  44  68  76  66  58  44  46  94  84
                  mults   64  70  60  78  76  54  76  68  76  62  56  44  38  34  40  bases -127..127
    SNorm Low     tables  44  44  90  38  36  46  18  44  68  76  66  58  44  46  94  84
                  mults   64  70  60  78  76  54  76  68  76  62  56  44  38  34  40  bases -127..127
    SNorm Normal  tables  42  40  82  42  42  46  18  38  76  78  64  58  44  46 100  80
                  mults   62  70  62  78  74  56  74  72  70  68  50  44  40  34  42  bases -127..127
    SNorm High    tables  40  44  82  32  38  54  22  34  76  80  64  62  46  46  98  78
                  mults   62  64  68  68  78  62  68  80  64  64  48  50  38  40  42  bases -127..127
    SNorm Highest tables  40  44  82  32  38  54  22  34  76  80  64  62  46  46  98  78
                  mults   62  64  68  68  78  62  68  80  64  64  48  50  38  40  42  bases -127..127
    alpha Lowest  tables  21  25  39  14  24  29  12  23  26  40  21  49  17  25  34  49
                  mults   31  34  30  43  33  36  35  33  41  25  25  19  27  19  17  bases 0..254
    alpha Low     tables  21  25  39  14  24  29  12  23  26  40  21  49  17  25  34  49
                  mults   31  34  30  43  33  36  35  33  41  25  25  19  27  19  17  bases 0..254
    alpha Normal  tables  19  22  35  16  22  30  13  20  27  44  25  47  18  23  37  50
                  mults   31  32  31  42  32  34  36  37  38  25  28  19  26  20  17  bases 0..253
    alpha High    tables  18  21  31  17  22  28  15  21  28  48  24  46  19  23  40  47
                  mults   30  33  30  41  33  34  37  33  40  25  29  19  26  20  18  bases 0..251
    alpha Highest tables  18  21  31  17  22  28  15  21  28  48  24  46  19  23  40  47
                  mults   30  33  30  41  33  34  37  33  40  25  29  19  26  20  18  bases 0..251

Largest error of a flat colour in ETC1 (flat_colours(), 512 colours) per level: 6 5 3 3 3.
"""
import functools

import numpy as np

import oracle_lib as O

ETC1, RGB, A1, A8, R11, RG11 = 37, 38, 39, 40, 41, 42
UNORM, SNORM = 0, 1
LEVELS = (0, 1, 2, 3, 4)                       # Lowest .. Highest
INDIVIDUAL, DIFFERENTIAL, T, H, PLANAR = 0, 1, 2, 3, 4
MODE_NAMES = ("individual", "differential", "T", "H", "planar")
# the seven classes of a colour block: mode and, for the two modes that have one, the flip bit
CLASS_NAMES = ("individual flip 0", "individual flip 1", "differential flip 0", "differential flip 1", "T", "H",
               "planar")
EAC_MOD = np.array([[-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12],
                    [-2, -4, -6, -13, 1, 3, 5, 12], [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10],
                    [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10], [-2, -6, -8, -10, 1, 5, 7, 9],
                    [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
                    [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8],
                    [-3, -5, -7, -9, 2, 4, 6, 8]], np.int64)
EAC_TABLE_13 = EAC_MOD[13]
ETC_MOD = np.array([[2, 8], [5, 17], [9, 29], [13, 42], [18, 60], [24, 80], [33, 106], [47, 183]], np.int64)


def block_bytes(fmt):
    return 16 if int(fmt) in (A8, RG11) else 8


# ---- classifiers --------------------------------------------------------------------------------------------

def colour_part(payload, fmt):
    """the 8-byte colour blocks of a payload (RGBA8: the second half of every 16-byte block)"""
    p = np.asarray(payload, np.uint8)
    return p.reshape(-1, 16)[:, 8:] if int(fmt) == A8 else p.reshape(-1, 8)


def mode_of(blocks8, a1=False):
    """-> (mode, flip) of every 8-byte colour block, from the overflow rules of the ETC2 specification: with the
    differential bit (bit 33) set, R + dR outside 0..31 is T, else G + dG outside is H, else B + dB outside is
    planar.  a1: RGB8A1, where bit 33 is the opaque flag and every block is laid out as differential."""
    b = np.asarray(blocks8, np.uint8).reshape(-1, 8).astype(np.int64)
    hi = (b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8) | b[:, 3]
    sx = lambda v: np.where(v >= 4, v - 8, v)                                   # noqa: E731
    r, g, bl = ((hi >> 27) & 31) + sx((hi >> 24) & 7), ((hi >> 19) & 31) + sx((hi >> 16) & 7), \
        ((hi >> 11) & 31) + sx((hi >> 8) & 7)
    out = lambda v: (v < 0) | (v > 31)                                          # noqa: E731
    mode = np.where(out(r), T, np.where(out(g), H, np.where(out(bl), PLANAR, DIFFERENTIAL)))
    if not a1:
        mode = np.where((hi >> 1) & 1, mode, INDIVIDUAL)
    return mode, hi & 1


def etc_mode(block8):
    """one block: 0 individual / differential, 1 T, 2 H, 3 planar"""
    return max(int(mode_of(block8)[0][0]) - 1, 0)


def class_of(blocks8, a1=False):
    """0..6, see CLASS_NAMES"""
    mode, flip = mode_of(blocks8, a1)
    return np.where(mode <= DIFFERENTIAL, 2*mode + flip, mode + 2)


def class_counts(payload, fmt):
    return np.bincount(class_of(colour_part(payload, fmt), int(fmt) == A1), minlength=7)


def opaque_flag(blocks8):
    """RGB8A1: bit 33"""
    return (np.asarray(blocks8, np.uint8).reshape(-1, 8)[:, 3] >> 1) & 1


def eac_fields(blocks8, signed=False):
    """-> (base, multiplier, table) of every 8-byte EAC block; the base as int8 for signed"""
    b = np.asarray(blocks8, np.uint8).reshape(-1, 8)
    base = b[:, 0].view(np.int8).astype(np.int64) if signed else b[:, 0].astype(np.int64)
    return base, (b[:, 1] >> 4).astype(np.int64), (b[:, 1] & 15).astype(np.int64)


# ---- sources ------------------------------------------------------------------------------------------------

def _grid(wide):
    return (36, 12) if wide else (28, 16)                                       # blocks across, blocks down


@functools.lru_cache(maxsize=None)
def _colour_source(seed, per_class, wide):
    rng = np.random.default_rng(seed)
    bx, by = _grid(wide)
    per = -(-bx*by//7) if wide else per_class
    kept = [np.zeros((0, 8), np.uint8)]*7
    while min(len(k) for k in kept) < per:
        draw = rng.integers(0, 256, (4096, 8), dtype=np.uint8)
        cls = class_of(draw)
        kept = [np.concatenate([k, draw[cls == c]])[:per] for c, k in enumerate(kept)]
    blocks = np.concatenate(kept)
    blocks = blocks[rng.permutation(len(blocks))][:bx*by]
    img = O.decode_etc(blocks.reshape(-1), RGB, 4*bx, 4*by)
    img.setflags(write=False)
    return img


def colour_source(seed=7, per_class=64, wide=False):
    """Random 8-byte blocks bucketed by the seven classes until each holds per_class, shuffled, laid out 28 x 16
    and decoded as ETC2 RGB: a 112 x 64 RGBA8 image (alpha 255) every block of which one of the modes expresses
    exactly.  wide: 36 x 12 blocks (144 x 48), for crops up to 33 blocks wide.  Read-only; copy before writing."""
    return _colour_source(seed, per_class, bool(wide))


def _selector_bytes(sel):
    """(n, 16) selectors in the block's own texel order -> the (n, 6) bytes of their 48 bits"""
    bits = np.zeros(len(sel), np.uint64)
    for k in range(16):
        bits |= sel[:, k].astype(np.uint64) << np.uint64(45 - 3*k)
    return np.stack([(bits >> np.uint64(40 - 8*i)) & np.uint64(255) for i in range(6)], axis=1).astype(np.uint8)


def _random_eac_blocks(rng, n, kind):
    """n random EAC blocks (kind 0 alpha8, 1 R11, 2 signed R11), balanced so that a re-encode reaches everything:
    multipliers 1..15 in equal counts, in random order; three blocks in four take a table whose modifiers times the
    multiplier fit the value range and a base that centres them there (a block whose values clamp comes back with a
    smaller multiplier: unbalanced, 14 and 15 all but vanish), the fourth keeps its random table and base; a signed
    base of -128 becomes -127.  Eight blocks of multiplier 1 are replaced by blocks at the ends of the range, the
    only ones a search places its base at: four flat at the lowest value, four at the highest (signed: the highest
    with the values three and, in two of them, six base steps below it -- a search that tries few bases finds 127
    exact for the first two, one that tries many finds a lower base exact for them but not for the others)."""
    b = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    mult = rng.permutation(np.arange(n) % 15 + 1)
    table = (b[:, 1] & 15).astype(np.int64)
    step, lo, hi = (1, 0, 255) if kind == 0 else ((8, 0, 2047) if kind == 1 else (8, -1023, 1023))
    off = 4 if kind == 1 else 0
    neg, pos = -EAC_MOD[:, 3], EAC_MOD[:, 7]
    centred, pick_t, pick_b = rng.random(n) < 0.75, rng.random(n), rng.random(n)
    for i in np.flatnonzero(centred):
        fits = np.flatnonzero((neg + pos)*mult[i]*step <= hi - lo + step)      # (one step of slack: 17*15*8 = 2046 - 6)
        if table[i] not in fits:
            table[i] = fits[int(pick_t[i]*len(fits))]
        t, m = table[i], mult[i]
        first = -((off - lo - neg[t]*m*step)//step)                             # the bases that clamp nothing
        last = (hi - off - pos[t]*m*step)//step
        base = first + int(pick_b[i]*(last - first + 1)) if first <= last else (first + last)//2
        b[i, 0] = int(base) & 255
    b[:, 1] = (mult << 4) | table
    if kind == 2:
        b[b[:, 0] == 0x80, 0] = 0x81
    ends = np.flatnonzero(mult == 1)[:8]
    sel = np.full((8, 16), 3)
    if kind == 2:
        sel[4:6], sel[6:8] = np.tile([0, 4], 8), np.tile([0, 1, 4, 4], 4)
    else:
        sel[4:] = 7
    b[ends, 0] = np.repeat([0x81, 0x7F] if kind == 2 else [0, 255], 4)
    b[ends, 1] = 1 << 4                                                          # multiplier 1, table 0
    b[ends, 2:] = _selector_bytes(sel)
    return b


@functools.lru_cache(maxsize=None)
def _a1_source(wide):
    img = colour_source(A1_SEED, wide=wide).copy()
    hit = np.random.default_rng(3).random(img.shape[:2]) < 0.25
    hit[:16] = False
    img[..., 3] = np.where(hit, 0, 255)
    img.setflags(write=False)
    return img


A1_SEED = 55


def a1_source(wide=False):
    """the colour source (seed A1_SEED: the first seed whose oracle payloads meet the floors of check_mode_counts at
    every level from Low up) with alpha 0 on a quarter of the texels, default_rng(3); the first 16 rows stay opaque"""
    return _a1_source(bool(wide))


@functools.lru_cache(maxsize=None)
def _a8_source(seed, wide):
    bx, by = _grid(wide)
    blocks = np.zeros((bx*by, 16), np.uint8)
    blocks[:, :8] = _random_eac_blocks(np.random.default_rng(seed), bx*by, 0)
    img = colour_source(wide=wide).copy()
    img[..., 3] = O.decode_etc(blocks.reshape(-1), A8, 4*bx, 4*by)[..., 3]
    img.setflags(write=False)
    return img


def a8_source(seed=5, wide=False):
    """the colour source under the alpha of random 8-bit EAC blocks (multipliers balanced), decoded as RGBA8"""
    return _a8_source(seed, bool(wide))


@functools.lru_cache(maxsize=None)
def _eac_source(typ, seed, wide):
    signed = int(typ) == SNORM
    bx, by = _grid(wide)
    blocks = _random_eac_blocks(np.random.default_rng(seed), bx*by, 2 if signed else 1)
    v = O.decode_eac(blocks.reshape(-1), R11, 4*bx, 4*by, int(typ))[..., 0]
    img = np.zeros((4*by, 4*bx, 4), np.float32)
    img[..., 0] = v.astype(np.float32)/np.float32(1023 if signed else 2047)
    img[..., 1] = img[:, ::-1, 0]
    img[..., 3] = 1
    img.setflags(write=False)
    return img


EAC_SEEDS = {UNORM: 1, SNORM: 2}


def eac_source(typ, seed=None, wide=False):
    """Random EAC blocks (multipliers 1..15 in equal counts) decoded as R11 into channel 0 of a float32 image as
    v/2047 (signed: v/1023, which the loader rounds back to v), the same values mirrored left to right in channel 1."""
    return _eac_source(int(typ), EAC_SEEDS[int(typ)] if seed is None else seed, bool(wide))


def r11_levels(img, typ, nch=1):
    """the loader of EAC R11 / RG11, stated once in numpy: float32 -> the integers the search sees.  NaN is 0, the
    clamp comes first, the product is taken in float32 and rounds half away from zero."""
    signed = int(typ) == SNORM
    f = np.asarray(img, np.float32)[..., :nch]
    f = np.where(np.isnan(f), np.float32(0), f)
    f = np.clip(f, np.float32(-1 if signed else 0), np.float32(1))
    x = (f*np.float32(1023 if signed else 2047)).astype(np.float64)
    return (np.sign(x)*np.floor(np.abs(x) + 0.5)).astype(np.int64)


def unorm8_levels(img):
    """the colour loader: NaN is 0, clamp to 0..1, the product with 255 in float32, half rounds up"""
    f = np.asarray(img, np.float32)
    f = np.where(np.isnan(f), np.float32(0), f)
    f = np.clip(f, np.float32(0), np.float32(1))
    return np.floor((f*np.float32(255)).astype(np.float64) + 0.5).astype(np.uint8)


def as_float(img8):
    return img8.astype(np.float32)/np.float32(255)


# ---- counts -------------------------------------------------------------------------------------------------

def check_mode_counts(payload, fmt, quality):
    """payload of colour_source() (ETC1, ETC2 RGB, RGBA8) or a1_source() (RGB8A1): the floors of the module
    docstring.  T and H exist from Low up; ETC1 has individual and differential only."""
    fmt = int(fmt)
    cnt = class_counts(payload, fmt)
    if fmt == A1:
        blocks = colour_part(payload, fmt)
        mode, opq = mode_of(blocks, True)[0], opaque_flag(blocks)
        got = {(o, m): int(((opq == o) & (mode == m)).sum()) for o in (0, 1) for m in (DIFFERENTIAL, T, H, PLANAR)}
        assert got[0, PLANAR] == 0, "planar cannot be punch-through: %s" % got
        if quality >= 1:
            floors = {(1, DIFFERENTIAL): 31, (1, T): 25, (1, H): 26, (1, PLANAR): 16,
                      (0, DIFFERENTIAL): 112, (0, T): 173, (0, H): 11}
            assert all(got[k] >= v for k, v in floors.items()), "(opaque, mode) -> blocks: %s" % got
        return
    need = [0, 1, 2, 3] if fmt == ETC1 else ([0, 1, 2, 3, 6] if quality == 0 else range(7))
    absent = [c for c in range(7) if c not in need]
    assert all(cnt[c] >= 35 for c in need) and all(cnt[c] == 0 for c in absent), \
        "blocks per class %s: %s" % (CLASS_NAMES, list(cnt))


def check_eac_counts(payload, typ):
    """payload of eac_source(typ) as R11 or RG11: every table in >= 8 blocks, every multiplier 1..15 in >= 4, and
    bases at both ends of their range"""
    signed = int(typ) == SNORM
    base, mult, table = eac_fields(payload, signed)
    tc, mc = np.bincount(table, minlength=16), np.bincount(mult, minlength=16)
    assert (tc >= 8).all(), "blocks per table: %s" % list(tc)
    assert mc[0] == 0 and (mc[1:] >= 4).all(), "blocks per multiplier: %s" % list(mc)
    if signed:
        assert (base == -127).any() and (base == 127).any() and not (base == -128).any()
    else:
        assert (base <= 8).any() and (base >= 249).any()


# ---- flat laws ----------------------------------------------------------------------------------------------

def _flat_blocks(values, bx):
    """(n, C) per-block values -> (4 by, 4 bx, C) image of flat blocks, the last value repeated to fill the grid"""
    values = np.asarray(values)
    by = -(-len(values)//bx)
    grid = np.concatenate([values, np.repeat(values[-1:], bx*by - len(values), axis=0)]).reshape(by, bx, -1)
    return np.ascontiguousarray(np.repeat(np.repeat(grid, 4, axis=0), 4, axis=1))


def check_flat_alpha_law(encode, quality):
    """flat alpha 0..255 over a flat grey through RGBA8 decodes exactly"""
    v = np.arange(256, dtype=np.uint8)
    img = _flat_blocks(np.stack([v[::-1], v[::-1], v[::-1], v], axis=1), 16)
    dec = O.decode_etc(encode(img, A8, UNORM, quality), A8, 64, 64)
    assert np.array_equal(dec[..., 3], img[..., 3])


def check_flat_r11_law(encode, fmt, typ, quality):
    """flat blocks of every 11-bit level decode within 4 (decoded values sit on a grid of 8)"""
    signed = int(typ) == SNORM
    v = np.arange(-1023, 1024) if signed else np.arange(0, 2048)
    f = (v/(1023.0 if signed else 2047.0)).astype(np.float32)
    img = _flat_blocks(np.stack([f, f[::-1], 0*f, 0*f + 1], axis=1).astype(np.float32), 64)
    nch = 2 if int(fmt) == RG11 else 1
    want = r11_levels(img, typ, nch)
    assert np.array_equal(want[::4, ::4, 0].reshape(-1)[:len(v)], v)
    dec = O.decode_eac(encode(img, fmt, typ, quality), fmt, img.shape[1], img.shape[0], int(typ))
    worst = int(np.abs(dec - want).max())
    assert worst <= 4, worst


# the oracle's own largest error of a flat colour in ETC1 per level (individual 4 + 4 bits or differential 5 bits
# with the smallest modifier 2): measured on the 512 colours below
ETC1_FLAT_MAX = {0: 6, 1: 5, 2: 3, 3: 3, 4: 3}


def flat_colours():
    rgb = np.random.default_rng(3).integers(0, 256, (512, 3), dtype=np.uint8)
    return _flat_blocks(np.concatenate([rgb, np.full((512, 1), 255, np.uint8)], axis=1), 32)


def check_flat_colour_law(encode, fmt, quality):
    """512 random flat colours decode within 2 per channel in the ETC2 formats (planar: 6 / 7 / 6 bits), within
    ETC1_FLAT_MAX in ETC1"""
    img = flat_colours()
    dec = O.decode_etc(encode(img, fmt, UNORM, quality), fmt, img.shape[1], img.shape[0])
    worst = int(np.abs(dec[..., :3].astype(np.int64) - img[..., :3]).max())
    assert worst <= (ETC1_FLAT_MAX[quality] if int(fmt) == ETC1 else 2), worst
    assert (dec[..., 3] == 255).all()


# ---- flat bounds --------------------------------------------------------------------------------------------

def _blocks(a):
    """(4 by, 4 bx, C) -> (by*bx, 16, C)"""
    h, w, c = a.shape
    return a.reshape(h//4, 4, w//4, 4, c).transpose(0, 2, 1, 3, 4).reshape(-1, 16, c)


def flat_bound_rgb(img):
    """Per 4x4 block (sides multiples of 4): the error of the differential block with both base colours at the
    block mean (rounded, then rounded to 5 bits as the encoder's walk starts: (mean*31 + 127)/255), zero deltas, the
    best of the 8 tables and the best selector per texel.  Unit weights, int64."""
    px = _blocks(np.asarray(img)[..., :3].astype(np.int64))
    mean = (2*px.sum(axis=1) + 16)//32
    q = (mean*31 + 127)//255
    base = (q << 3) | (q >> 2)                                                  # (n, 3)
    mods = np.concatenate([ETC_MOD, -ETC_MOD], axis=1)                          # (8 tables, 4 modifiers)
    paint = np.clip(base[:, None, None, :] + mods[None, :, :, None], 0, 255)    # (n, 8, 4, 3)
    d = paint[:, :, :, None, :] - px[:, None, None, :, :]                       # (n, 8, 4, 16, 3)
    return (d*d).sum(axis=4).min(axis=2).sum(axis=2).min(axis=1)


def block_error_rgb(img, decoded):
    d = _blocks(np.asarray(img)[..., :3].astype(np.int64)) - _blocks(np.asarray(decoded)[..., :3].astype(np.int64))
    return (d*d).sum(axis=(1, 2))


def _over(e, b):
    worse = e > b
    ratio = float((e[worse]/np.maximum(b[worse], 1)).max()) if worse.any() else 0.0
    return int(worse.sum()), ratio


def over_flat_bound_rgb(payload, img, fmt):
    """-> (blocks whose colour error exceeds the flat block's, worst ratio); img: RGBA8, opaque for RGB8A1"""
    dec = O.decode_etc(payload, fmt, img.shape[1], img.shape[0])
    return _over(block_error_rgb(img, dec), flat_bound_rgb(img))


def flat_bound_eac(vals, kind):
    """vals (4 by, 4 bx) integers; kind 0 alpha8, 1 R11, 2 signed R11.  Per block the error of table 13
    (-1 -2 -3 -10 0 1 2 9), multiplier 1, base at the rounded mean (in base units: 8 levels, the unsigned grid
    sits at 8 base + 4), the best modifier per texel."""
    v = _blocks(np.asarray(vals, np.int64)[..., None])[..., 0]                  # (n, 16)
    s = v.sum(axis=1)
    if kind == 0:
        base = np.clip((2*s + 16)//32, 0, 255)
        dec = np.clip(base[:, None] + EAC_TABLE_13[None], 0, 255)
    elif kind == 1:
        base = np.clip((2*(s - 64) + 128)//256, 0, 255)                         # round((mean - 4)/8)
        dec = np.clip(8*base[:, None] + 4 + 8*EAC_TABLE_13[None], 0, 2047)
    else:
        base = np.clip((2*s + 128)//256, -127, 127)
        dec = np.clip(8*base[:, None] + 8*EAC_TABLE_13[None], -1023, 1023)
    d = dec[:, None, :] - v[:, :, None]
    return (d*d).min(axis=2).sum(axis=1)


def over_flat_bound_eac(payload, vals, typ, fmt=R11):
    """-> (blocks over the bound, worst ratio).  fmt R11 / RG11: vals (h, w, channels) 11-bit levels; fmt RGBA8:
    vals (h, w) alpha bytes."""
    h, w = vals.shape[:2]
    if int(fmt) == A8:
        dec, vals, kind = O.decode_etc(payload, A8, w, h)[..., 3:4].astype(np.int64), vals.reshape(h, w, 1), 0
    else:
        dec, kind = O.decode_eac(payload, fmt, w, h, int(typ)).astype(np.int64), 2 if int(typ) == SNORM else 1
    n, ratio = 0, 0.0
    for c in range(dec.shape[2]):
        d = _blocks(dec[..., c:c + 1] - vals[..., c:c + 1])[..., 0]
        k, r = _over((d*d).sum(axis=1), flat_bound_eac(vals[..., c], kind))
        n, ratio = n + k, max(ratio, r)
    return n, ratio


def noise_image(seed=5, w=128, h=64):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def bound_sources():
    """the three opaque RGBA8 sources of the colour flat bound: [(name, image)]"""
    import cuttlefish_amd.synth as synth
    return [("modes", colour_source()), ("photo", synth.photo(128, 64, seed=5, alpha=False)),
            ("noise", noise_image())]


# the flat bound holds from these levels up (ETC1: High; why not Normal, and the levels below: DESIGN.md 4.4)
BOUND_FROM = {ETC1: 3, RGB: 2, A1: 2, A8: 2}


# ---- rounding boundaries --------------------------------------------------------------------------------------

def _around(ties):
    ties = np.asarray(ties, np.float32)
    return np.stack([np.nextafter(ties, np.float32(-np.inf)), ties, np.nextafter(ties, np.float32(np.inf))],
                    axis=1).reshape(-1)


def _specials():
    one = np.float32(1)
    sp = np.array([0.0, 1.0, -1.0, np.nextafter(np.float32(0), -one), np.nextafter(one, np.float32(2)),
                   np.nextafter(-one, np.float32(-2)), -0.0, np.inf, -np.inf, 0.0, 0.0], np.float32)
    sp.view(np.uint32)[-2:] = (0x7FC00000, 0xFFC00000)                          # NaN of both signs
    return sp


def unorm8_boundaries():
    """float32: for every k the tie (k + 0.5)/255 and its two neighbours, then 0, 1, -1, the values just outside
    the clamps, -0, +-Inf and NaN of both signs"""
    k = np.arange(255, dtype=np.float64)
    return np.concatenate([_around((k + 0.5)/255), _specials()])


def r11_boundaries(snorm):
    k = np.arange(1023 if snorm else 2047, dtype=np.float64)
    t = (k + 0.5)/(1023 if snorm else 2047)
    return np.concatenate([_around(t), _around(-t), _specials()] if snorm else [_around(t), _specials()])


def unorm8_boundary_image():
    """one boundary value per flat block, in all four channels (alpha: 127.5/255 is RGB8A1's punch-through
    threshold and RGBA8 codes the byte exactly)"""
    v = unorm8_boundaries()
    return _flat_blocks(np.stack([v, v, v, v], axis=1), 28)


def r11_boundary_image(snorm):
    v = r11_boundaries(snorm)
    return _flat_blocks(np.stack([v, v[::-1], 0*np.nan_to_num(v, posinf=0, neginf=0), np.ones_like(v)], axis=1), 64)


def _same_blocks(a, b, bs, what):
    bad = np.flatnonzero((a.reshape(-1, bs) != b.reshape(-1, bs)).any(axis=1))
    assert bad.size == 0, "%s: %d blocks differ, first %s" % (what, bad.size, bad[:10])


def check_unorm8_law(encode, fmt, quality):
    """The float32 boundary image encodes to the bytes of its numpy-rounded RGBA8 image; the decoded alpha is the
    rounded byte itself (RGBA8), its comparison with 128 (RGB8A1) or 255.  -> the payload"""
    f = unorm8_boundary_image()
    u8 = unorm8_levels(f)
    assert u8[0, 0, 0] == 0 and u8[0, 4, 0] == 1 and u8[0, 8, 0] == 1         # below the tie, the tie, above it
    p = encode(f, fmt, UNORM, quality)
    _same_blocks(p, encode(u8, fmt, UNORM, quality), block_bytes(fmt), "float32 boundaries against their bytes")
    alpha = O.decode_etc(p, fmt, f.shape[1], f.shape[0])[..., 3]
    want = u8[..., 3] if int(fmt) == A8 else (np.where(u8[..., 3] >= 128, 255, 0) if int(fmt) == A1 else 255)
    assert np.array_equal(alpha, np.broadcast_to(want, alpha.shape))
    return p


def check_r11_law(encode, fmt, typ, quality):
    """The float32 boundary image encodes to the bytes of the image of its numpy-rounded levels (v/2047 or v/1023,
    which round back to v), and decodes within 4 of them.  -> the payload"""
    signed = int(typ) == SNORM
    f = r11_boundary_image(signed)
    nch = 2 if int(fmt) == RG11 else 1
    lv = r11_levels(f, typ, 2)
    g = f.copy()
    g[..., :2] = lv.astype(np.float32)/np.float32(1023 if signed else 2047)
    assert np.array_equal(r11_levels(g, typ, 2), lv)
    p = encode(f, fmt, typ, quality)
    _same_blocks(p, encode(g, fmt, typ, quality), block_bytes(fmt), "float32 boundaries against their levels")
    dec = O.decode_eac(p, fmt, f.shape[1], f.shape[0], int(typ))
    worst = int(np.abs(dec - lv[..., :nch]).max())
    assert worst <= 4, worst
    return p


SPECIALS = np.array([np.nan, np.nan, np.inf, -np.inf, -0.0, -1.0, 1e9, 6e-8], np.float32)


def sprinkle_specials(img, seed=3, share=0.02):
    """float32 copy of an RGBA image with `share` of the values of all four channels replaced by +-NaN, +-Inf, -0,
    -1, 1e9 and 6e-8"""
    rng = np.random.default_rng(seed)
    sp = SPECIALS.copy()
    sp.view(np.uint32)[:2] = (0x7FC00000, 0xFFC00000)
    f = as_float(img) if img.dtype == np.uint8 else np.array(img, np.float32)
    hit = rng.random(f.shape) < share
    return np.where(hit, sp[rng.integers(0, sp.size, f.shape)], f).astype(np.float32)
