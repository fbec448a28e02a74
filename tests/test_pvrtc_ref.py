"""The numpy PVRTC1 4 bpp twin (tests/pvrtc_ref.py) against the format's published rules: hand-derived decode
vectors, the twiddled block order, payload sizes, and the encoder's guarantees (lossless on representable constants,
error never rising from sweep to sweep or from level to level)."""
import os

import numpy as np
import pytest

import pvrtc_ref as P

FIX = os.path.join(os.path.dirname(__file__), "golden", "pvrtc_photos.npz")


def blocks(colour_words, mod_words):
    """payload of an 8 x 8 surface (2 x 2 blocks) from per-block words given in raster order"""
    cw = np.broadcast_to(np.asarray(colour_words, np.uint64), (4,))
    mw = np.broadcast_to(np.asarray(mod_words, np.uint64), (4,))
    out = np.zeros(4, np.uint64)
    for i in range(4):
        out[int(P.twiddle(i % 2, i // 2, 2, 2))] = mw[i] | cw[i] << np.uint64(32)
    return np.frombuffer(out.astype("<u8").tobytes(), np.uint8)


def test_hand_vector_modulation_mode0():
    d = P.decode(blocks(0xFFFF8000, 0xE4E4E4E4), 8, 8)
    for y in range(8):
        assert list(d[y, :, 0]) == [0, 95, 159, 255] * 2
        assert (d[y, :, 0] == d[y, :, 1]).all() and (d[y, :, 0] == d[y, :, 2]).all()
        assert (d[y, :, 3] == 255).all()


def test_hand_vector_punch_through():
    d = P.decode(blocks(0xFFFF8001, 0xE4E4E4E4), 8, 8)
    for y in range(8):
        assert list(d[y, :, 0]) == [0, 127, 127, 255] * 2
        assert list(d[y, :, 3]) == [255, 255, 0, 255] * 2


def test_hand_vector_translucent_alpha():
    d = P.decode(blocks(0x00007FFE, 0), 8, 8)
    assert (d.reshape(-1, 4) == [255, 255, 255, 238]).all()


def test_hand_vector_centres_weights_wrap():
    d = P.decode(blocks([0x8000FC00, 0x80008000, 0x80008000, 0x80008000], 0), 8, 8)
    want = [127, 191, 255, 191, 127, 63, 0, 63]
    assert list(d[2, :, 0]) == want
    assert list(d[:, 2, 0]) == want


def test_rgb_format_decodes_opaque():
    d = P.decode(blocks(0x00007FFE, 0), 8, 8, P.RGB)
    assert (d[..., 3] == 255).all()


@pytest.mark.parametrize("bx, by, want", [
    (4, 2, [[0, 2, 4, 6], [1, 3, 5, 7]]),
    (2, 4, [[0, 2], [1, 3], [4, 6], [5, 7]]),
    (4, 4, [[0, 2, 8, 10], [1, 3, 9, 11], [4, 6, 12, 14], [5, 7, 13, 15]]),
])
def test_twiddle_order(bx, by, want):
    ys, xs = np.mgrid[0:by, 0:bx]
    assert P.twiddle(xs, ys, bx, by).tolist() == want


@pytest.mark.parametrize("w, h, n", [(1, 1, 32), (4, 4, 32), (16, 8, 64), (8, 32, 128), (64, 64, 2048)])
def test_payload_size(w, h, n):
    assert P.payload_size(w, h) == n
    assert P.encode(np.zeros((h, w, 4), np.uint8), P.RGB, 0).size == n


@pytest.mark.parametrize("fmt", [P.RGB, P.RGBA])
@pytest.mark.parametrize("colour", [(165, 74, 99, 255), (0, 255, 33, 255)])
@pytest.mark.parametrize("quality", range(5))
def test_representable_constant_is_lossless(fmt, colour, quality):
    """opaque colours whose channels are 5-bit values expanded to 8 bits, blue also a 4-bit one (colour A holds
    blue in 4 bits): (165, 74, 99) = 5-bit (20, 9, 12), 12 = 4-bit 6; (0, 255, 33) = (0, 31, 4), 4 = 4-bit 2"""
    img = np.empty((16, 16, 4), np.uint8)
    img[...] = colour
    p = P.encode(img, fmt, quality)
    assert sum(P.sse(p, img, fmt)) == 0


def _crops():
    z = np.load(FIX)
    return [(P.RGB, c) for c in z["rgb"][:3]] + [(P.RGBA, c) for c in z["rgba"]]


def test_sse_never_rises_over_sweeps_and_levels():
    """The Highest run's sweeps contain every lower level's (each level runs the sweeps of the level below first):
    the error after each sweep bounds the next, and the payload of each level decodes to its trace entry."""
    for fmt, crop in _crops():
        crop = crop[:64, :64]
        trace = []
        P.encode(crop, fmt, 4, trace=trace)
        assert all(b <= a for a, b in zip(trace, trace[1:])), trace
        chans = 3 if fmt == P.RGB else 4
        last = None
        for q in range(5):
            s = sum(P.sse(P.encode(crop, fmt, q), crop, fmt)[:chans])
            assert s == trace[len(P.LEVEL_SWEEPS[q])]
            assert last is None or s <= last
            last = s


# ---- one vector per colour field ---------------------------------------------------------------------------
# Every block carries the same colour word, so the four bilinear weights (total 16) hit equal colours: the sum
# is 16 v, RGB (16v >> 6) + (16v >> 1) = (v >> 2) + 8v, the 5-bit value with its top 3 bits repeated below; alpha
# (16a >> 4) + 16a = 17a, the 4-bit value repeated.  Modulation word 0 is value 0 everywhere (pure A), 0xFFFFFFFF
# value 3 everywhere (pure B), mode 0.  Shorter fields widen by repeating their top bits first:
#   5-bit 21 = 10101            -> 10101 101 = 173       5-bit 19 = 10011 -> 10011 100 = 156
#   5-bit 13 = 01101            -> 01101 011 = 107
#   4-bit 10 = 1010 -> 1010 1 = 21 -> 173                4-bit 9 = 1001 -> 1001 1 = 19 -> 156
#   4-bit 13 = 1101 -> 1101 1 = 27 = 11011 -> 11011 110 = 222
#   3-bit 5 = 101 -> 101 10 = 22 = 10110 -> 10110 101 = 181      (colour A's translucent blue)
#   3-bit alpha 5 = 101 -> 4-bit 1010 = 10 -> 17 * 10 = 170
# Layout: A opaque = 1 R5 G5 B4 in bits 15..1, A translucent = 0 A3 R4 G4 B3; B opaque = 1 R5 G5 B5 in bits
# 31..16, B translucent = 0 A3 R4 G4 B4.  An opaque colour has alpha 255; every field left at 0 decodes to 0.
# (name, colour word, modulation word, decoded RGBA in the RGBA format)
FIELD_VECTORS = [
    ("A opaque R5", 0x8000 | 21 << 10, 0, (173, 0, 0, 255)),
    ("A opaque G5", 0x8000 | 19 << 5, 0, (0, 156, 0, 255)),
    ("A opaque B4", 0x8000 | 13 << 1, 0, (0, 0, 222, 255)),
    ("A translucent A3", 5 << 12, 0, (0, 0, 0, 170)),
    ("A translucent R4", 10 << 8, 0, (173, 0, 0, 0)),
    ("A translucent G4", 9 << 4, 0, (0, 156, 0, 0)),
    ("A translucent B3", 5 << 1, 0, (0, 0, 181, 0)),
    ("B opaque R5", 0x80000000 | 21 << 26, 0xFFFFFFFF, (173, 0, 0, 255)),
    ("B opaque G5", 0x80000000 | 19 << 21, 0xFFFFFFFF, (0, 156, 0, 255)),
    ("B opaque B5", 0x80000000 | 13 << 16, 0xFFFFFFFF, (0, 0, 107, 255)),
    ("B translucent A3", 5 << 28, 0xFFFFFFFF, (0, 0, 0, 170)),
    ("B translucent R4", 10 << 24, 0xFFFFFFFF, (173, 0, 0, 0)),
    ("B translucent G4", 9 << 20, 0xFFFFFFFF, (0, 156, 0, 0)),
    ("B translucent B4", 13 << 16, 0xFFFFFFFF, (0, 0, 222, 0)),
]

# Two colours, both translucent, no two channels alike:
#   A = A3 3, R4 10, G4 4, B3 5: alpha 3 -> 4-bit 6 -> 102; R 173; G 0100 -> 01000 = 8 -> 01000 010 = 66; B 181
#   B = A3 6, R4 2, G4 13, B4 9: alpha 6 -> 12 -> 204; R 0010 -> 00100 = 4 -> 00100 001 = 33; G 222; B 156
#   A word 3 << 12 | 10 << 8 | 4 << 4 | 5 << 1 = 0x3A4A, B word 6 << 12 | 2 << 8 | 13 << 4 | 9 = 0x62D9
# A8 = (173, 66, 181, 102), B8 = (33, 222, 156, 204); texel = (A8 (8 - w) + B8 w) >> 3.
#   mode 0, value 1, w = 3: R (865 + 99) >> 3 = 120, G (330 + 666) >> 3 = 124, B (905 + 468) >> 3 = 171,
#                           A (510 + 612) >> 3 = 140
#   mode 0, value 2, w = 5: R (519 + 165) >> 3 = 85, G (198 + 1110) >> 3 = 163, B (543 + 780) >> 3 = 165,
#                           A (306 + 1020) >> 3 = 165
#   mode 1, value 1, w = 4: R 206 >> 1 = 103, G 288 >> 1 = 144, B 337 >> 1 = 168, A 306 >> 1 = 153
#   mode 1, value 2: the same RGB, punched through: alpha 0
# (colour word, modulation word, decoded RGBA in the RGBA format)
TWO_COLOUR_VECTORS = [
    (0x62D93A4A, 0x55555555, (120, 124, 171, 140)),
    (0x62D93A4A, 0xAAAAAAAA, (85, 163, 165, 165)),
    (0x62D93A4B, 0x55555555, (103, 144, 168, 153)),
    (0x62D93A4B, 0xAAAAAAAA, (103, 144, 168, 0)),
]


def check_constant_vector(decode, word, mod, want):
    """decode(payload, fmt) of an 8 x 8 surface of equal blocks is the constant `want`; alpha 255 in the RGB format"""
    p = blocks(word, mod)
    got = decode(p, P.RGBA).reshape(-1, 4)
    assert (got == want).all(), (hex(word), got[0].tolist(), want)
    got = decode(p, P.RGB).reshape(-1, 4)
    assert (got == tuple(want[:3]) + (255,)).all(), (hex(word), got[0].tolist(), want)


@pytest.mark.parametrize("name, word, mod, want", FIELD_VECTORS, ids=[v[0] for v in FIELD_VECTORS])
def test_hand_vector_colour_field(name, word, mod, want):
    check_constant_vector(lambda p, fmt: P.decode(p, 8, 8, fmt), word, mod, want)


def test_hand_vector_two_colours_both_modes():
    for word, mod, want in TWO_COLOUR_VECTORS:
        check_constant_vector(lambda p, fmt: P.decode(p, 8, 8, fmt), word, mod, want)


# ---- float sources -----------------------------------------------------------------------------------------
# (value, byte): round(clamp(f, 0, 1) * 255) with the product rounded to float32 and halves away from zero, NaN and
# everything not above 0 -> 0.  The ties sit at (k + 0.5) / 255: the float32 nearest to it and its two neighbours,
# each byte worked out in exact rational arithmetic (the product of a 24-bit value by 255 rounded to 24 bits).
SPECIALS_F32 = [
    (float("nan"), 0), (float("inf"), 255), (float("-inf"), 0), (-0.0, 0), (-1.0, 0), (1.0 + 2.0 ** -20, 255),
    (2.0, 255), (65504.0, 255), (1e-40, 0), (1.0, 255),
    (float.fromhex("0x1.010100p-9"), 0), (float.fromhex("0x1.010102p-9"), 1), (float.fromhex("0x1.010104p-9"), 1),
    (float.fromhex("0x1.818180p-8"), 1), (float.fromhex("0x1.818182p-8"), 2), (float.fromhex("0x1.818184p-8"), 2),
    (float.fromhex("0x1.fffffep-2"), 127), (0.5, 128), (float.fromhex("0x1.000002p-1"), 128),
    (float.fromhex("0x1.929290p-1"), 200), (float.fromhex("0x1.929292p-1"), 201),
    (float.fromhex("0x1.929294p-1"), 201),
    (float.fromhex("0x1.fefefcp-1"), 254), (float.fromhex("0x1.fefefep-1"), 255),
    (float.fromhex("0x1.feff00p-1"), 255),
]
# (float16 bit pattern, byte): NaN, +Inf, -Inf, -0, -1, 2, 65504, the smallest subnormal, then the float16 nearest
# to (k + 0.5) / 255 and its neighbours for k = 0, 1, 127, 200, 254 (0x3800 is 0.5 -> 127.5 -> 128)
SPECIALS_F16 = [
    (0x7E00, 0), (0x7C00, 255), (0xFC00, 0), (0x8000, 0), (0xBC00, 0), (0x4000, 255), (0x7BFF, 255), (0x0001, 0),
    (6147, 0), (6148, 0), (6149, 1), (7685, 1), (7686, 1), (7687, 2), (14335, 127), (0x3800, 128), (14337, 128),
    (14921, 200), (14922, 200), (14923, 201), (15355, 254), (15356, 255), (15357, 255),
]


def special_source(dtype):
    """16 x 16 source whose 1024 channel values cycle through the specials (an odd count, so every special lands
    in all four channels), and the bytes the load pass must make of them"""
    if dtype == np.float32:
        vals = np.array([v for v, _ in SPECIALS_F32], np.float32)
        want = [b for _, b in SPECIALS_F32]
    else:
        vals = np.array([v for v, _ in SPECIALS_F16], np.uint16).view(np.float16)
        want = [b for _, b in SPECIALS_F16]
    assert len(want) % 2 == 1
    idx = np.arange(16 * 16 * 4) % len(want)
    return vals[idx].reshape(16, 16, 4), np.array(want, np.int64)[idx].reshape(16, 16, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_to_rgba8_float_specials(dtype):
    src, want = special_source(dtype)
    assert src.dtype == dtype
    got = P.to_rgba8(src)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (src[tuple(bad[0])], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- tiling: a periodic surface encodes to its tile's blocks ------------------------------------------------
def tile_content(tw, th, kind, seed):
    """tw x th RGBA8 tile whose content wraps smoothly (every term has the tile's period), with noise on top;
    kind: opaque, graded alpha, or cut-out alpha"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:th, 0:tw]
    fx, fy = 2 * np.pi * xx / tw, 2 * np.pi * yy / th
    img = np.empty((th, tw, 4), np.float64)
    img[..., 0] = 128 + 80 * np.sin(fx) * np.cos(fy) + 30 * np.sin(3 * fy)
    img[..., 1] = 120 + 100 * np.cos(fx + fy)
    img[..., 2] = 100 + 60 * np.sin(2 * fx) + 60 * np.cos(fy)
    img[..., 3] = 255
    if kind == "graded":
        img[..., 3] = 128 + 127 * np.sin(fx) * np.sin(fy)
    elif kind == "cutout":
        img[..., 3] = np.where(((xx // 3) + (yy // 5)) % 3 == 0, 0, 255)
    img[..., :3] += rng.integers(-12, 13, (th, tw, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def retile(tile_payload, tw, th, w, h):
    """the payload of a w x h surface that repeats a tw x th tile, from the tile's payload: block (x, y) of the
    surface is block (x mod bx, y mod by) of the tile, each at its own twiddled index"""
    bx, by = P.grid(tw, th)
    BX, BY = P.grid(w, h)
    assert tw % 8 == 0 and th % 8 == 0 and w % tw == 0 and h % th == 0
    tile = np.frombuffer(np.ascontiguousarray(tile_payload).tobytes(), "<u8")
    ys, xs = np.mgrid[0:BY, 0:BX]
    out = np.empty(BX * BY, "<u8")
    out[P.twiddle(xs, ys, BX, BY)] = tile[P.twiddle(xs % bx, ys % by, bx, by)]
    return out


def first_block_difference(got, want, tw, th, w, h):
    """None, or a description of the first block (raster order) at which two w x h payloads differ"""
    BX, BY = P.grid(w, h)
    g = np.frombuffer(np.ascontiguousarray(got).tobytes(), "<u8")
    e = np.frombuffer(np.ascontiguousarray(want).tobytes(), "<u8")
    if g.size == e.size and np.array_equal(g, e):
        return None
    if g.size != e.size:
        return "payload of %d blocks, expected %d" % (g.size, e.size)
    ys, xs = np.mgrid[0:BY, 0:BX]
    tw_idx = P.twiddle(xs, ys, BX, BY)
    bad = np.argwhere(g[tw_idx] != e[tw_idx])
    y, x = (int(v) for v in bad[0])
    i = int(tw_idx[y, x])
    return "%d blocks differ; first at block (%d, %d), tile block (%d, %d): got %016x, expected %016x" % (
        len(bad), x, y, x % (tw // 4), y % (th // 4), int(g[i]), int(e[i]))


TILINGS = [(8, 8, 32, 32), (8, 8, 64, 16), (16, 8, 64, 32), (16, 16, 32, 128), (32, 16, 64, 128), (32, 16, 64, 64)]


@pytest.mark.parametrize("fmt", [P.RGB, P.RGBA])
@pytest.mark.parametrize("tw, th, w, h", TILINGS)
def test_tiled_surface_encodes_to_its_tile(fmt, tw, th, w, h):
    """PVRTC1 wraps around and every encoder pass is local and translation-invariant under shifts by an even
    number of blocks, so a surface that repeats a tile (sides multiples of 8 px) must encode to the tile's own
    blocks.  The GPU tests at full size rest on this; here the twin proves it on sizes it can encode whole."""
    for i, q in enumerate((0, 2, 4)):
        tile = tile_content(tw, th, ("cutout", "graded", "opaque")[(i + tw // 8 + fmt) % 3], seed=tw * th + q)
        big = np.tile(tile, (h // th, w // tw, 1))
        want = retile(P.encode(tile, fmt, q), tw, th, w, h)
        diff = first_block_difference(P.encode(big, fmt, q), want, tw, th, w, h)
        assert diff is None, (q, diff)
