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
