"""GPU parity of BC7's exact instruction trims: the 4-entry selector search has no mode-6 lane exchange (it is
entered only when no active lane of the wave is a mode-6 lane), the channel set of a fit is folded into the
rotation's v_perm_b32 selector (a selector byte 0x0C reads as zero) instead of an AND per texel, and 1/n of a
subset of n texels comes from a table of the 16 correctly rounded quotients instead of an IEEE division.  Every
payload must equal the CPU oracle's, block by block; what a tile has to exercise is a condition on the oracle's
output alone (checked without a GPU in the *_exercise tests).

Quality 0 (Lowest) tries the single-subset modes only, so mode 1 cannot occur there: the mixed tile's condition
"modes 6 and 1 both occur" is asserted from quality 1 up, "mode 6 occurs" at every level."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)

# the two- and three-subset partition tables of the format (texel i of a block: bit i / bit pair i)
K_PART2 = (
    0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
    0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
    0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
    0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22)
K_PART3 = (
    0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050,
    0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250,
    0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500,
    0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200,
    0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50,
    0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600,
    0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000,
    0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254)
PART_BITS = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}      # partition field of the modes that have one (it follows the mode bit)


def _sizes2(p):
    n = bin(K_PART2[p]).count("1")
    return (16 - n, n)


def _sizes3(p):
    v = [(K_PART3[p] >> (2 * i)) & 3 for i in range(16)]
    return tuple(v.count(s) for s in range(3))


ALL_SIZES2 = frozenset(n for p in range(64) for n in _sizes2(p))
ALL_SIZES3 = frozenset(n for p in range(64) for n in _sizes3(p))


def _modes(payload):
    """BC7 mode of every block: the position of the lowest set bit of its first byte"""
    b0 = payload.reshape(-1, 16)[:, 0].astype(np.int64)
    return np.array([(int(v) & -int(v)).bit_length() - 1 for v in b0])


def _header(payload):
    b = payload.reshape(-1, 16).astype(np.int64)
    return b[:, 0] | (b[:, 1] << 8)


def _rotations(payload):
    """The two bits after the mode bit (the channel rotation of modes 4 and 5)"""
    return (_header(payload) >> (_modes(payload) + 1)) & 3


def _subset_sizes(payload):
    """Subset sizes of the two- and of the three-subset blocks of a payload"""
    s2, s3 = set(), set()
    for mode, hd in zip(_modes(payload), _header(payload)):
        if int(mode) in PART_BITS:
            p = (int(hd) >> (int(mode) + 1)) & ((1 << PART_BITS[int(mode)]) - 1)
            if mode in (0, 2):
                s3.update(_sizes3(p))
            else:
                s2.update(_sizes2(p))
    return s2, s3


# ---- tiles (each built once, read-only) ----

@functools.lru_cache(maxsize=None)
def _ramp_bands(seed):
    """128x64, four bands of 32 columns.  Each has a ramp along x in one channel and a ramp along y in another,
    +-2 noise on both, the rest constant: mode 5 with the y channel as its scalar plane, a different one per band
    (alpha, red, green, blue), so that every rotation wins somewhere."""
    rng = np.random.default_rng(seed)
    width, height = 128, 64
    y, x = np.mgrid[0:height, 0:width]
    img = np.empty((height, width, 4), np.uint8)
    img[..., :3] = 40
    img[..., 3] = 255
    xr = (x % 32 * 3 + 40 + rng.integers(-2, 3, x.shape)).clip(0, 255)
    yr = (3 * y + 30 + rng.integers(-2, 3, x.shape)).clip(0, 255)
    for band, (cx, cy) in enumerate(((0, 3), (1, 0), (2, 1), (0, 2))):
        cols = slice(32 * band, 32 * band + 32)
        img[:, cols, cx] = xr[:, cols]
        img[:, cols, cy] = yr[:, cols]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _mixed(width, height, seed):
    """Photo content, per-block noise, flat and two-tone blocks and a 4-row alpha ramp in one tile"""
    rng = np.random.default_rng(seed)
    img = synth.photo2(width, height, seed=seed).copy()
    img[..., 3] = 255
    for by in range(height // 4):
        for bx in range(width // 4):
            k = (by * 5 + bx * 3 + seed) % 6
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            if k == 0:
                blk[..., :3] = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
            elif k == 1:
                blk[..., :3] = rng.integers(0, 256, 3, dtype=np.uint8)
            elif k == 2:
                two = rng.integers(0, 256, (2, 3), dtype=np.uint8)
                sel = (np.arange(16).reshape(4, 4) * 7 + bx) % 3 == 0
                blk[..., :3] = np.where(sel[..., None], two[0], two[1])
    a0 = height // 2 // 4 * 4
    img[a0:a0 + 4, :, 3] = np.linspace(0, 255, width).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _noise(seed, alpha):
    """64x64 noise, opaque or with random alpha"""
    img = np.random.default_rng(seed).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    if not alpha:
        img[..., 3] = 255
    img.setflags(write=False)
    return img


RAMP_SEED, MIXED_SEED = 1, 1
NOISE_TILES = ((1, False), (2, True))          # (seed, alpha)
NOISE_CASES = [(seed, alpha, quality) for seed, alpha in NOISE_TILES for quality in (2, 4)]


@functools.lru_cache(maxsize=None)
def _ref(kind, seed, alpha, quality, srgb):
    """The oracle's payload of one case: computed once, shared by the exercise and the parity tests"""
    img = {"ramps": lambda: _ramp_bands(seed), "mixed": lambda: _mixed(96, 64, seed), "noise": lambda: _noise(seed, alpha),
           "ragged": lambda: _mixed(72, 52, seed)[:50, :70]}[kind]()
    ref = O.encode(np.ascontiguousarray(img), BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return np.ascontiguousarray(img), ref


def _check(ctx, case):
    img, ref = _ref(*case)
    quality, srgb = case[3], case[4]
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    got = ctx.encode([img], make_params(Format.BC7, Type.UNorm, quality, **kw))[0]
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "blocks differ: %s" % bad[:10]


# ---- what the tiles exercise: conditions on the oracle's output alone (no GPU) ----

@pytest.mark.parametrize("quality", [2, 3])
def test_ramp_bands_exercise(quality):
    """More than half the blocks are mode 5 (2-bit indices on both planes: the 4-entry search), every rotation among them"""
    _, ref = _ref("ramps", RAMP_SEED, False, quality, False)
    m, r = _modes(ref), _rotations(ref)
    assert (m == 5).mean() > 0.5, np.bincount(m, minlength=8)
    assert set(r[m == 5].tolist()) == {0, 1, 2, 3}, np.bincount(r[m == 5], minlength=4)


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quality", [0, 1, 2, 3, 4])
def test_mixed_tile_exercise(quality, srgb):
    """Mode 6 (the search that keeps the exchange) next to mode 1 (from quality 1 up: Lowest has no partitions),
    and blocks with alpha"""
    img, ref = _ref("mixed", MIXED_SEED, False, quality, srgb)
    m = _modes(ref)
    assert (m == 6).any(), np.bincount(m, minlength=8)
    if quality >= 1:
        assert (m == 1).any(), np.bincount(m, minlength=8)
    assert (img[..., 3] != 255).any()


def test_noise_tiles_exercise():
    """Over the noise cases: modes 4 and 5 with a non-zero rotation, one of modes 0 / 2, one of modes 1 / 3 / 7 (every
    channel set a fit can code), and winners whose subsets have every size the partition tables can produce."""
    rot4, rot5, mall, s2, s3 = set(), set(), set(), set(), set()
    for seed, alpha, quality in NOISE_CASES:
        _, ref = _ref("noise", seed, alpha, quality, False)
        m, r = _modes(ref), _rotations(ref)
        rot4.update(r[m == 4].tolist())
        rot5.update(r[m == 5].tolist())
        mall.update(m.tolist())
        a, b = _subset_sizes(ref)
        s2 |= a
        s3 |= b
    assert rot4 - {0} and rot5 - {0}, (rot4, rot5)
    assert mall & {0, 2} and mall & {1, 3, 7}, mall
    assert s2 == ALL_SIZES2, sorted(ALL_SIZES2 - s2)
    assert s3 == ALL_SIZES3, sorted(ALL_SIZES3 - s3)


# ---- parity ----

@pytest.mark.gpu
@pytest.mark.parametrize("quality", [2, 3])
def test_ramp_bands(gpu_ctx, quality):
    """4-entry search without the exchange, under every rotation"""
    _check(gpu_ctx, ("ramps", RAMP_SEED, False, quality, False))


@pytest.mark.gpu
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quality", [0, 1, 2, 3, 4])
def test_mixed_tile(gpu_ctx, quality, srgb):
    """The search that must keep the exchange: a pair where one half holds a mode-6 candidate and the other does not"""
    _check(gpu_ctx, ("mixed", MIXED_SEED, False, quality, srgb))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,alpha,quality", NOISE_CASES)
def test_noise_tiles(gpu_ctx, seed, alpha, quality):
    """Selector fold under every channel set; 1/n for every subset size"""
    _check(gpu_ctx, ("noise", seed, alpha, quality, False))


@pytest.mark.gpu
def test_ragged_edge(gpu_ctx):
    """70x50: the last block column and row are replicated edges, 18 block columns"""
    _check(gpu_ctx, ("ragged", 71, False, 2, False))
