"""GPU parity of BC7's byte-packed endpoint arithmetic (csrc/bc7_packed.h): the quantiser clamps in float and inserts
each field into its word with one conversion, code words are dequantised four bytes at a time, and the quantised
refit window forms its q - 1 / q / q + 1 candidates as whole words and decides their validity from q == 0 and
q == qmax.  Every payload must equal the CPU oracle's, block by block, no block left out.

Three 64x64 tiles (256 blocks each): a mixed one (smooth, edged, noisy and alpha-ramped blocks), a saturated one
(every block holds 0 and 255 in every channel beside mid-tones) and a two-colour one (exactly two colours per block,
so every refit lands on or next to the ends of the field range).  What they must exercise is a condition on the
oracle's output alone, asserted without a GPU in the *_exercise tests: every mode from High up and the modes Normal
can choose (every (colour bits, alpha bits, p-bit kind) the quantiser sees), both values of a per-endpoint and of
mode 1's shared p-bit, and winning endpoint fields equal to 0 and to 2^bits - 1 (the window's out-of-range candidates)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params

BC7 = int(Format.BC7)

# per mode: subsets, partition bits, rotation bits, index-selector bits, colour bits, alpha bits, p-bits per endpoint, shared p-bits
MODES = {0: (3, 4, 0, 0, 4, 0, 1, 0), 1: (2, 6, 0, 0, 6, 0, 0, 1), 2: (3, 6, 0, 0, 5, 0, 0, 0), 3: (2, 6, 0, 0, 7, 0, 1, 0),
         4: (1, 0, 2, 1, 5, 6, 0, 0), 5: (1, 0, 2, 0, 7, 8, 0, 0), 6: (1, 0, 0, 0, 7, 7, 1, 0), 7: (2, 6, 0, 0, 5, 5, 1, 0)}


def _parse(block):
    """(mode, fields, bits of each field, p-bits, kind) of one 16-byte block: `fields` are the endpoint fields in
    stream order (colours then alpha), `kind` 1 for per-endpoint p-bits, 2 for shared ones, 0 for none."""
    v = int.from_bytes(bytes(block), "little")
    mode = (v & -v).bit_length() - 1
    ns, pb, rb, isb, cb, ab, epb, spb = MODES[mode]
    pos = mode + 1 + pb + rb + isb
    fields, widths = [], []
    for bits, count in ((cb, 3), (ab, 1 if ab else 0)):
        for _ in range(count * 2 * ns):
            fields.append((v >> pos) & ((1 << bits) - 1))
            widths.append(bits)
            pos += bits
    npb = 2 * ns if epb else (ns if spb else 0)
    pbits = [(v >> (pos + i)) & 1 for i in range(npb)]
    return mode, fields, widths, pbits, 1 if epb else (2 if spb else 0)


@functools.lru_cache(maxsize=None)
def _mixed(seed):
    """Smooth gradients, hard edges, noise and an alpha ramp, block by block"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:64, 0:64]
    img = np.empty((64, 64, 4), np.uint8)
    img[..., 0] = (2 * x + y + 20).clip(0, 255)
    img[..., 1] = (3 * y + 30 + 8 * np.sin(x / 3.0)).clip(0, 255)
    img[..., 2] = (200 - x - 2 * y).clip(0, 255)
    img[..., 3] = 255
    for by in range(16):
        for bx in range(16):
            k = (by * 7 + bx * 3 + seed) % 8
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            if k == 0:      # noise
                blk[..., :3] = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
            elif k == 1:    # an edge between two noisy regions, along a random direction
                a, b = rng.integers(0, 256, (2, 3))
                d = rng.integers(-2, 3, 2)
                side = (np.arange(4)[:, None] * d[0] + np.arange(4)[None, :] * d[1] + rng.integers(-3, 4)) > 0
                blk[..., :3] = (np.where(side[..., None], a, b) + rng.integers(-6, 7, (4, 4, 3))).clip(0, 255)
            elif k == 2:    # three regions
                cols = rng.integers(0, 256, (3, 3))
                reg = (np.arange(16).reshape(4, 4) * int(rng.integers(1, 6)) // 5) % 3
                blk[..., :3] = (cols[reg] + rng.integers(-4, 5, (4, 4, 3))).clip(0, 255)
            elif k == 3:    # alpha ramp over smooth colour
                blk[..., 3] = (np.arange(16).reshape(4, 4) * int(rng.integers(4, 17)) + int(rng.integers(0, 16))).clip(0, 255)
            elif k == 4:    # noisy alpha over an edge
                blk[..., 3] = rng.integers(0, 256, (4, 4), dtype=np.uint8)
                blk[:, 2:, :3] = rng.integers(0, 256, 3, dtype=np.uint8)
            elif k == 5:    # alpha uncorrelated with a smooth colour
                blk[..., 3] = np.where(rng.random((4, 4)) < 0.5, int(rng.integers(0, 128)), int(rng.integers(128, 256)))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _saturated(seed):
    """Every block holds 0 and 255 in every channel beside mid-tones"""
    rng = np.random.default_rng(seed)
    img = rng.integers(64, 192, (64, 64, 4), dtype=np.uint8)
    for by in range(16):
        for bx in range(16):
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].reshape(16, 4)
            for c in range(4):
                lo, hi = rng.choice(16, 2, replace=False)
                blk[lo, c] = 0
                blk[hi, c] = 255
            img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = blk.reshape(4, 4, 4)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _two_colour(seed):
    """Exactly two colours per block (alpha included in every third block), in a random pattern"""
    rng = np.random.default_rng(seed)
    img = np.empty((64, 64, 4), np.uint8)
    for by in range(16):
        for bx in range(16):
            two = rng.integers(0, 256, (2, 4))
            if (by * 16 + bx) % 4 == 0:        # the ends of the byte range themselves
                two = rng.choice([0, 255], (2, 4))
                two[1, :3] = 255 - two[0, :3]
            if (by + bx) % 3:
                two[:, 3] = 255
            sel = rng.random((4, 4)) < 0.5
            sel[0, 0], sel[3, 3] = False, True
            img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = np.where(sel[..., None], two[0], two[1])
    img.setflags(write=False)
    return img


TILES = {"mixed": _mixed, "saturated": _saturated, "two_colour": _two_colour}
SEEDS = {"mixed": 1, "saturated": 1, "two_colour": 1}
CASES = [(q, False, "u8") for q in range(5)] + [(q, True, "u8") for q in (2, 3, 4)] + [(2, False, "f32")]


@functools.lru_cache(maxsize=None)
def _ref(tile, quality, srgb, ptype):
    """Source and oracle payload of one case: computed once, shared by the exercise and the parity tests"""
    img = np.ascontiguousarray(TILES[tile](SEEDS[tile]))
    if ptype == "f32":
        img = (img.astype(np.float64) / 255.0).astype(np.float32)
    ref = O.encode(img, BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    img.setflags(write=False)
    ref.setflags(write=False)
    return img, ref


def _blocks(tile, quality, srgb=False, ptype="u8"):
    return [_parse(b) for b in _ref(tile, quality, srgb, ptype)[1].reshape(-1, 16)]


# ---- what the tiles exercise: conditions on the oracle's output alone (no GPU) ----

def test_tiles_are_what_they_say():
    sat = _saturated(SEEDS["saturated"]).reshape(16, 4, 16, 4, 4).transpose(0, 2, 1, 3, 4).reshape(256, 16, 4)
    assert (sat.min(axis=1) == 0).all() and (sat.max(axis=1) == 255).all()
    assert ((sat > 0) & (sat < 255)).any(axis=1).all()
    two = _two_colour(SEEDS["two_colour"]).reshape(16, 4, 16, 4, 4).transpose(0, 2, 1, 3, 4).reshape(256, 16, 4)
    assert all(len(np.unique(b, axis=0)) == 2 for b in two)
    mixed = _mixed(SEEDS["mixed"])
    assert (mixed[..., 3] != 255).any() and (mixed[..., 3] == 255).any()


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quality", [3, 4])
def test_mixed_tile_every_mode_exercise(quality, srgb):
    """From High up every mode wins somewhere: every (colour bits, alpha bits, p-bit kind) the quantiser sees"""
    modes = {b[0] for b in _blocks("mixed", quality, srgb)}
    assert modes == set(range(8)), sorted(modes)


@pytest.mark.parametrize("srgb", [False, True])
def test_mixed_tile_normal_modes_exercise(srgb):
    """Normal: modes 1, 3, 5, 6, a three-subset mode and mode 4 (the second pass's candidates)"""
    modes = {b[0] for b in _blocks("mixed", 2, srgb)}
    assert {1, 3, 4, 5, 6} <= modes and modes & {0, 2}, sorted(modes)


@pytest.mark.parametrize("quality,srgb,ptype", CASES)
def test_mixed_tile_pbits_exercise(quality, srgb, ptype):
    """Both values of a per-endpoint p-bit at every level, and of mode 1's shared p-bit from Low up (Lowest has no
    partitions)"""
    blocks = _blocks("mixed", quality, srgb, ptype)
    own = {p for b in blocks if b[4] == 1 for p in b[3]}
    assert own == {0, 1}, own
    if quality >= 1:
        shared = {p for b in blocks if b[0] == 1 for p in b[3]}
        assert shared == {0, 1}, shared


@pytest.mark.parametrize("tile", ["saturated", "two_colour"])
@pytest.mark.parametrize("quality,srgb,ptype", [c for c in CASES if c[0] >= 2])
def test_field_range_ends_exercise(tile, quality, srgb, ptype):
    """Some winning endpoint field equals 0 and some equals 2^bits - 1: there the window's q - 1 / q + 1 is out of range"""
    blocks = _blocks(tile, quality, srgb, ptype)
    at_zero = sum(any(f == 0 for f in b[1]) for b in blocks)
    at_max = sum(any(f == (1 << w) - 1 for f, w in zip(b[1], b[2])) for b in blocks)
    assert at_zero >= 1 and at_max >= 1, (at_zero, at_max)


# ---- parity ----

@pytest.mark.gpu
@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("quality,srgb,ptype", CASES)
def test_payload_equals_oracle(gpu_ctx, tile, quality, srgb, ptype):
    img, ref = _ref(tile, quality, srgb, ptype)
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    got = gpu_ctx.encode([img], make_params(Format.BC7, Type.UNorm, quality, **kw))[0]
    assert got.size == ref.size == 256 * 16
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "%d blocks differ: %s" % (bad.size, bad[:10])
