"""Shared BC6H cases (plain numpy + the CPU oracle's decoder; no GPU): the reference statement of the
half loader, the block error in the encoder's own metric, the constant-block bound, and the sources
whose payloads reach every mode and every rounding boundary.  Used by tests/test_bc6h_cases.py (the
oracle alone) and tests/test_gpu_bc6h_modes.py (the HIP kernel).

Blocks per mode 1..14 of the oracle's payload of mode_complete_source(typ) (seed 2024, 32 x 28 = 896
blocks, 64 per mode in the source).  The HIP kernel's payload is byte-equal, so these are its counts too:

    type    level      1   2   3   4   5   6   7   8   9  10  11  12  13  14
    UFloat  Lowest     0   0   0   0   0   0   0   0   0   0 341 157 334  64
    UFloat  Low       70  28  80  53  46  57  57  32  35 182  81  48  63  64
    UFloat  Normal    68  28  80  53  46  57  57  32  35 181  82  48  65  64
    UFloat  High      68  28  80  53  46  57  57  32  35 181  82  48  65  64
    UFloat  Highest   68  28  80  53  46  57  57  32  35 181  82  48  65  64
    Float   Lowest     0   0   0   0   0   0   0   0   0   0 319 175 338  64
    Float   Low       68  31  82  52  46  56  72  40  39 152  77  53  64  64
    Float   Normal    68  32  81  53  46  56  71  39  39 151  79  53  64  64
    Float   High      68  32  81  53  46  56  71  39  39 151  79  53  64  64
    Float   Highest   68  32  81  53  46  56  71  39  39 151  79  53  64  64
"""
import numpy as np

import oracle_lib as O

UFLOAT, FLOAT = 4, 5
LEVELS = (0, 1, 2, 3, 4)                       # Lowest .. Highest
MAX_HALF = 0x7BFF                              # largest finite half

# mode 1..14 -> (header bits, header value)
MODE_HEADERS = {1: (2, 0b00), 2: (2, 0b01), 3: (5, 0b00010), 4: (5, 0b00110), 5: (5, 0b01010), 6: (5, 0b01110),
                7: (5, 0b10010), 8: (5, 0b10110), 9: (5, 0b11010), 10: (5, 0b11110), 11: (5, 0b00011),
                12: (5, 0b00111), 13: (5, 0b01011), 14: (5, 0b01111)}


def mode_of(payload):
    """mode 1..14 of every 16-byte block (0 for a reserved header)."""
    b0 = np.asarray(payload, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    five = np.zeros(32, np.int64)
    for m, (bits, val) in MODE_HEADERS.items():
        if bits == 5:
            five[val] = m
    return np.where((b0 & 3) == 0, 1, np.where((b0 & 3) == 1, 2, five[b0 & 31]))


def mode_counts(payload):
    """blocks per mode: index m = mode m (index 0: reserved headers)"""
    return np.bincount(mode_of(payload), minlength=15)


def half_ints(bits, signed):
    """The loader, stated once: half bit patterns -> the integers the encoder measures errors in.  Magnitude
    min(bits & 0x7FFF, 0x7BFF) (Inf and NaN clamp to the largest finite half); UFloat: sign set -> 0; Float:
    sign set -> -magnitude (so -0 is 0)."""
    b = np.asarray(bits).astype(np.int64)
    mag = np.minimum(b & 0x7FFF, MAX_HALF)
    neg = (b >> 15) & 1
    if signed:
        return np.where(neg == 1, -mag, mag)
    return np.where(neg == 1, 0, mag)


def half_bits(img):
    """(h, w, >=3) float16 -> (h, w, 3) uint16 bit patterns of RGB"""
    return np.ascontiguousarray(np.asarray(img)[..., :3]).view(np.uint16)


def rgba16f(bits_rgb):
    """(h, w, 3) uint16 half bit patterns -> RGBA16F image with alpha 1"""
    bits_rgb = np.asarray(bits_rgb, np.uint16)
    img = np.empty(bits_rgb.shape[:2] + (4,), np.uint16)
    img[..., :3] = bits_rgb
    img[..., 3] = 0x3C00
    return img.view(np.float16)


def mode_complete_source(typ, seed=2024, bx=32, by=28):
    """by x bx random 16-byte blocks, block (r, c) under the header of mode ((r + c) % 14) + 1, decoded by the
    oracle's decoder: every 4x4 block of the image is exactly representable in its mode, and any crop 14
    blocks wide holds every mode."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, (by, bx, 16), dtype=np.uint8)
    for r in range(by):
        for c in range(bx):
            bits, val = MODE_HEADERS[((r + c) % 14) + 1]
            blocks[r, c, 0] = (int(blocks[r, c, 0]) & ~((1 << bits) - 1) & 0xFF) | val
    dec = O.decode_bc6h(blocks.reshape(-1), 4*bx, 4*by, int(typ))
    return rgba16f(dec.view(np.uint16))


def _blocks(a):
    """(4 by, 4 bx, 3) -> (by, bx, 16, 3)"""
    h, w = a.shape[:2]
    return a.reshape(h//4, 4, w//4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(h//4, w//4, 16, 3)


def flat_bound(img, typ):
    """Per 4x4 block (sides multiples of 4): the error of the constant block at the per-channel rounded mean
    floor((sum + 8)/16) of half_ints -- sum over texels and RGB of squared differences of half_ints."""
    hb = _blocks(half_ints(half_bits(img), int(typ) == FLOAT))
    mean = (hb.sum(axis=2, keepdims=True) + 8) >> 4
    return ((hb - mean)**2).sum(axis=(2, 3))


def block_error(img, decoded, typ):
    """The same metric between the source and a decoded payload ((h, w, 3) float16 of O.decode_bc6h)."""
    signed = int(typ) == FLOAT
    a = _blocks(half_ints(half_bits(img), signed))
    b = _blocks(half_ints(half_bits(decoded), signed))
    return ((a - b)**2).sum(axis=(2, 3))


def finite_halves(signed):
    """every finite half bit pattern: 31 744 non-negative ones, then (signed) the 31 744 negative ones"""
    pos = np.arange(0, MAX_HALF + 1, dtype=np.uint16)
    return np.concatenate([pos, pos | np.uint16(0x8000)]) if signed else pos


def flat_surfaces(values, width_blocks=256):
    """One grey flat 4x4 block per half bit pattern, width_blocks blocks per row, split into RGBA16F surfaces of at
    most 62 block rows (1024 x 248 texels); the last row of the last surface repeats the last value.
    -> list of (image, block values (by, bx))"""
    values = np.asarray(values, np.uint16)
    rows = -(-values.size//width_blocks)
    grid = np.full(rows*width_blocks, values[-1], np.uint16)
    grid[:values.size] = values
    grid = grid.reshape(rows, width_blocks)
    out = []
    for r0 in range(0, rows, 62):
        g = grid[r0:r0 + 62]
        out.append((flat_image(np.repeat(g[..., None], 3, axis=2)), g))
    return out


def flat_image(block_bits_rgb):
    """(by, bx, 3) uint16 -> RGBA16F image of flat 4x4 blocks"""
    return rgba16f(np.repeat(np.repeat(np.asarray(block_bits_rgb, np.uint16), 4, axis=0), 4, axis=1))


def flat_rgb_surface(typ, seed=7, n=64):
    """n x n flat blocks whose three channels are independent finite halves (non-negative for UFloat)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, MAX_HALF + 1, (n, n, 3)).astype(np.uint16)
    if int(typ) == FLOAT:
        bits |= (rng.integers(0, 2, (n, n, 3)).astype(np.uint16) << 15)
    return flat_image(bits)


def non_finite_flat(negative):
    """flat blocks of every Inf / NaN half 0x7C00..0x7FFF (or their negatives): 32 x 32 blocks"""
    bits = np.arange(0x7C00, 0x8000, dtype=np.uint16) | np.uint16(0x8000 if negative else 0)
    return flat_image(np.repeat(bits.reshape(32, 32, 1), 3, axis=2))


def bytes_flat():
    """all 256 byte values as flat grey blocks of an RGBA8 image (16 x 16 blocks), alpha 255"""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.repeat(np.repeat(v, 4, axis=0), 4, axis=1)[..., None].repeat(4, axis=2)
    img[..., 3] = 255
    return np.ascontiguousarray(img)


def bytes_as_half(img8):
    """the loader's 8-bit conversion: float32(v)/float32(255) rounded to half"""
    f = img8.astype(np.float32)/np.float32(255)
    return f.astype(np.float16)


def half_boundaries(signed=False, seed=11):
    """RGBA32F image 256 x 128 whose RGB hold the RNE boundaries of float32 -> half: for every pair of
    consecutive finite halves the midpoint (exact in float32) and its two float32 neighbours (95 229 values), NaNs
    of both signs with quiet and signalling payloads, +-Inf, +-0, 65520 (the first value that rounds to Inf) and
    the float32 below it, +-1e9, 2^-25 (half of the smallest denormal half: ties to 0), the float32 neighbours of
    2^-25 and 2^-24, and the smallest float32 denormal with its neighbours.  signed: the same values under random
    signs.  The rest of the image repeats 1.0."""
    h = np.arange(0, MAX_HALF, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float32)
    hi = (h + np.uint16(1)).view(np.float16).astype(np.float32)
    mid = (lo + hi)*np.float32(0.5)
    assert np.array_equal(mid.astype(np.float64), (lo.astype(np.float64) + hi.astype(np.float64))/2)
    ties = np.stack([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(np.inf))], axis=1).reshape(-1)
    nan_bits = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC12345, 0x7F800001, 0xFF800001, 0x7FA00000,
                         0xFFA00000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)
    one = np.float32(1)
    p25, p24, den = np.float32(2.0**-25), np.float32(2.0**-24), np.float32(2.0**-149)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 65520.0, np.nextafter(np.float32(65520), np.float32(0)),
                        1e9, -1e9, p25, np.nextafter(p25, np.float32(0)), np.nextafter(p25, one),
                        np.nextafter(p24, np.float32(0)), np.nextafter(p24, one), den, np.float32(0),
                        np.nextafter(den, one)], np.float32)
    vals = np.concatenate([ties, nan_bits, special]).astype(np.float32)
    assert ties.size == 95229
    w, hgt = 256, 128
    flat = np.ones(w*hgt*3, np.float32)
    flat[:vals.size] = vals
    if signed:
        rng = np.random.default_rng(seed)
        u = flat.view(np.uint32)
        u ^= (rng.integers(0, 2, u.size).astype(np.uint32) << np.uint32(31))
    img = np.ones((hgt, w, 4), np.float32)
    img[..., :3] = flat.reshape(hgt, w, 3)
    return img


def to_half(f32):
    """numpy's float32 -> half (round to nearest even; overflow to Inf, NaN stays NaN with its sign)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return f32.astype(np.float16)


def noise_image(seed=5, n=64, signed=False):
    """n x n log-uniform noise over 2^-14 .. 2^15 (RGBA16F), random signs where signed"""
    rng = np.random.default_rng(seed)
    f = np.exp2(rng.uniform(-14.0, 15.0, (n, n, 4)))
    if signed:
        f *= np.where(rng.random((n, n, 4)) < 0.5, -1.0, 1.0)
    f[..., 3] = 1.0
    return f.astype(np.float16)


def bound_sources(typ):
    """the three sources of the flat-bound check: [(name, RGBA16F image)]"""
    import cuttlefish_amd.synth as synth
    signed = int(typ) == FLOAT
    return [("mode_complete", mode_complete_source(typ)),
            ("hdr_probe", synth.hdr_probe(128, 128, seed=4, signed=False)),
            ("hdr_probe_signed", synth.hdr_probe(128, 128, seed=4, signed=True)),
            ("noise", noise_image(signed=signed))]


SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, -1.0, 1e9, -1e9, 6e-8, 65504.0], np.float32)


def sprinkle_specials(img, seed=3, share=0.02):
    """float32 copy of an RGBA image with `share` of its RGB values replaced by +-NaN, +-Inf, -0, -1, +-1e9,
    6e-8 and 65504"""
    rng = np.random.default_rng(seed)
    sp = SPECIALS.copy()
    sp.view(np.uint32)[1] = 0xFFC00000                      # -NaN: the sign bit set explicitly
    sp.view(np.uint32)[0] = 0x7FC00000
    f = np.array(img, np.float32)
    hit = rng.random(f.shape) < share
    hit[..., 3] = False
    pick = sp[rng.integers(0, sp.size, f.shape)]
    return np.where(hit, pick, f)


# ---- the laws, stated over any encoder: encode(img, typ, quality) -> payload bytes -------------------------

def decoded_ints(payload, img, typ):
    """half_ints of what the oracle's decoder reads from a payload of img's size"""
    dec = O.decode_bc6h(payload, img.shape[1], img.shape[0], int(typ))
    return half_ints(half_bits(dec), int(typ) == FLOAT)


def check_flat_law(encode, typ, quality):
    """Every finite half (grey), 64 x 64 three-channel flat blocks, negative (UFloat) and non-finite flat blocks
    decode to half_ints of the source, texel for texel."""
    signed = int(typ) == FLOAT
    cases = [img for img, _ in flat_surfaces(finite_halves(signed))]
    cases.append(flat_rgb_surface(typ))
    cases += [non_finite_flat(False), non_finite_flat(True)]
    if not signed:
        cases += [img for img, _ in flat_surfaces(finite_halves(True)[MAX_HALF + 1:])]     # negative -> 0
    for i, img in enumerate(cases):
        want = half_ints(half_bits(img), signed)
        got = decoded_ints(encode(img, typ, quality), img, typ)
        bad = np.argwhere(want != got)
        assert bad.size == 0, "flat case %d: %d texels differ, first at %s: source %d decoded %d" % (
            i, len(bad), bad[0], want[tuple(bad[0])], got[tuple(bad[0])])
    # spelled out, not through half_ints: the non-finite rows and the negative UFloat rows
    for neg in (False, True):
        img = non_finite_flat(neg)
        bits = half_bits(O.decode_bc6h(encode(img, typ, quality), 128, 128, int(typ)))
        want = (0xFBFF if neg else 0x7BFF) if signed else (0 if neg else 0x7BFF)
        assert (bits == want).all(), (neg, hex(int(bits.flat[np.flatnonzero(bits.reshape(-1) != want)[0]])))


def check_byte_law(encode, typ, quality):
    """All 256 byte values as flat blocks decode to half(float32(v)/float32(255)) exactly, and the payload is the
    payload of that half image."""
    img8 = bytes_flat()
    h = bytes_as_half(img8)
    p = encode(img8, typ, quality)
    assert np.array_equal(p, encode(h, typ, quality))
    assert np.array_equal(decoded_ints(p, h, typ), half_ints(half_bits(h), int(typ) == FLOAT))


def check_float32_law(encode, typ, quality):
    """encode(f32) == encode(numpy's RNE half of f32) on every rounding boundary"""
    f = half_boundaries(int(typ) == FLOAT)
    a, b = encode(f, typ, quality), encode(to_half(f), typ, quality)
    bad = np.flatnonzero((a.reshape(-1, 16) != b.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "blocks differ between the float32 source and its half: %s" % bad[:10]
    return a


def over_flat_bound(payload, img, typ):
    """-> (blocks whose error exceeds the flat block's, worst ratio)"""
    dec = O.decode_bc6h(payload, img.shape[1], img.shape[0], int(typ))
    e, b = block_error(img, dec, typ), flat_bound(img, typ)
    worse = e > b
    ratio = float((e[worse]/np.maximum(b[worse], 1)).max()) if worse.any() else 0.0
    return int(worse.sum()), ratio


def check_mode_counts(payload, quality):
    """the mode-complete source's payload: every mode in at least 16 blocks (Lowest: modes 11..14)"""
    cnt = mode_counts(payload)
    assert cnt[0] == 0
    need = range(11, 15) if quality == 0 else range(1, 15)
    assert all(cnt[m] >= 16 for m in need), "blocks per mode 1..14: %s" % list(cnt[1:])
