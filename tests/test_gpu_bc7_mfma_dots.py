"""GPU parity of BC7 with the selector search's cross terms on the matrix pipe (v_mfma_i32_4x4x4_16b_i8, the fit run with the
whole wave on) and the weight in a full byte of its keys (tenth step; mfma_entry_base and
key_row_weights in csrc/bc7_packed.h).  Every payload must equal the
CPU oracle's byte for byte, at levels 0..4, with both metrics (the perceptual instances keep their forms and are covered
as the untouched half), from an RGBA8 and from an RGBA32F source.

Tiles: the five of test_gpu_bc7_key_trims.py (photo 64 x 64 seed 6 with its alpha band, photo2 64 x 64, ragged 30 x 22,
odd 18 x 10 whose last block has no partner in its wave, the 16 x 16 flat "ties" tile) and
  signs    16 x 16: every texel's channels drawn from {0, 127, 128, 255} (seeded), half of the blocks with alpha below 255:
           the extremes of every dot product and the byte values on both sides of bit 7, where a key that lost its sign,
           or a weight byte that took a bit of the error, shows
  planes   16 x 16: blocks whose colour is flat in two channels while the third ramps along x and alpha along y, so that
           the two planes of modes 4 / 5 each carry one ramp; the rotations 1, 2 and 3 must all occur among the mode-5
           blocks of the Normal payload
The oracle's payloads are computed once per case and shared."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)
TILES = ("photo", "photo2", "ragged", "odd", "ties", "signs", "planes")
CASES = [(q, srgb) for srgb in (False, True) for q in range(5)]


def _ties():
    r = np.random.default_rng(77)
    img = np.empty((16, 16, 4), np.uint8)
    for by in range(4):
        for bx in range(4):
            c = r.integers(0, 256, 4)
            if (by + bx) % 2:
                c[3] = 255
            img[4*by:4*by + 4, 4*bx:4*bx + 4] = c
    return img


def _signs():
    r = np.random.default_rng(2024)
    img = np.array([0, 127, 128, 255], np.uint8)[r.integers(0, 4, (16, 16, 4))]
    for by in range(4):
        for bx in range(4):
            if (by + bx) % 2 == 0:
                img[4*by:4*by + 4, 4*bx:4*bx + 4, 3] = 255
    return img


def _planes():
    r = np.random.default_rng(5)
    img = np.empty((16, 16, 4), np.uint8)
    for by in range(4):
        for bx in range(4):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            ramp = (4*by + bx) % 3
            blk[:, :, :3] = r.integers(0, 256, 3)
            lo, hi = sorted(int(v) for v in r.choice(256, 2, replace=False))
            blk[:, :, ramp] = np.round(np.linspace(lo, hi, 4)).astype(np.uint8)[None, :]
            lo, hi = sorted(int(v) for v in r.choice(255, 2, replace=False))
            blk[:, :, 3] = np.round(np.linspace(lo, hi, 4)).astype(np.uint8)[:, None]
    return img


@functools.lru_cache(maxsize=None)
def _image(tile, ptype):
    if tile == "photo":
        img = synth.photo(64, 64, seed=6)
    elif tile == "photo2":
        img = synth.photo2(64, 64, seed=1)
    elif tile == "ragged":
        img = np.ascontiguousarray(synth.photo(64, 64, seed=3)[7:29, 11:41])
    elif tile == "odd":
        img = np.ascontiguousarray(synth.photo(64, 64, seed=3)[30:40, 40:58])
    elif tile == "ties":
        img = _ties()
    elif tile == "signs":
        img = _signs()
    else:
        img = _planes()
    if ptype == "f32":
        img = (img.astype(np.float64)/255.0).astype(np.float32)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(tile, ptype, quality, srgb):
    ref = O.encode(_image(tile, ptype), BC7, quality=quality, threads=4, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return ref


def _mode5_rotations(payload):
    """rotation field (bits 6..7 of the first byte) of every mode-5 block (first byte xx100000)"""
    first = payload.reshape(-1, 16)[:, 0]
    return sorted(set(int(b) >> 6 for b in first if (int(b) & 63) == 32))


def test_tile_shapes():
    s = _image("signs", "u8")
    assert s.shape == (16, 16, 4) and set(np.unique(s)) == {0, 127, 128, 255}
    opaque = [(s[4*by:4*by + 4, 4*bx:4*bx + 4, 3] == 255).all() for by in range(4) for bx in range(4)]
    assert sum(opaque) >= 8 and sum(not o for o in opaque) >= 7, opaque
    p = _image("planes", "u8")
    assert p.shape == (16, 16, 4)
    for by in range(4):
        for bx in range(4):
            blk = p[4*by:4*by + 4, 4*bx:4*bx + 4].astype(int)
            flat = [c for c in range(3) if (blk[:, :, c] == blk[0, 0, c]).all()]
            assert len(flat) == 2, (by, bx, flat)
            assert (blk[:, :, 3] == blk[:, :1, 3]).all() and blk[0, 0, 3] != blk[3, 0, 3]
    assert _image("odd", "u8").shape == (10, 18, 4) and _image("ragged", "u8").shape == (22, 30, 4)


def test_planes_tile_asks_for_every_rotation():
    """what the GPU assertion below rests on: the oracle's own Normal payload has mode-5 blocks of rotations 1, 2 and 3"""
    assert {1, 2, 3} <= set(_mode5_rotations(_ref("planes", "u8", 2, False)))


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, ptype, quality, srgb):
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    params = make_params(Format.BC7, Type.UNorm, quality, **kw)
    for tile in TILES:
        img, ref = _image(tile, ptype), _ref(tile, ptype, quality, srgb)
        got = gpu_ctx.encode([img], params)[0]      # a call of its own: surfaces of one call share a launch
        assert got.size == ref.size == ((img.shape[0] + 3)//4)*((img.shape[1] + 3)//4)*16
        bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
        assert bad.size == 0, "%s: blocks %s differ" % (tile, bad)
        if tile == "planes" and quality == 2 and not srgb:
            assert {1, 2, 3} <= set(_mode5_rotations(np.asarray(got))), _mode5_rotations(np.asarray(got))
