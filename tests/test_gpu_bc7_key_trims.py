"""GPU parity of BC7 with the key trims (ninth step; key_min_form in csrc/bc7_packed.h,
csrc/bc7_rcp.h): the
selector search's keys in minimum form, the reciprocals as v_rcp_f32 and a Newton step.  Every payload must equal the CPU oracle's byte for byte, at levels 0..4, with both
metrics, from an RGBA8 and from an RGBA32F source.

Tiles, the smallest at which a wrong tie-break, a wrong exchange between the halves of mode 6 or a wrong quotient can
show:
  photo    64 x 64 synth.photo with its alpha band: 256 blocks, enough for every lane role of both trips to win somewhere
  photo2   64 x 64 synth.photo2
  ragged   30 x 22: neither side a multiple of 4 (8 x 6 blocks from 7.5 x 5.5), edge replication on two sides
  odd      18 x 10: 5 x 3 blocks, odd counts both ways, so the last block of the launch has no partner in its wave
  ties     16 x 16 of flat blocks: both endpoints dequantise to the same colour, every palette entry is that colour and
           all entries tie for every texel (the weight decides), in both halves of mode 6
The oracle's payloads are computed once per case and shared.  At Normal the mode histogram of the payloads the GPU
returned is asserted: modes 1, 3, 5 and 6 win blocks of the two 64 x 64 tiles (synth.photo is smooth at this size and
gives modes 3 and 5, synth.photo2 the others), and mode 4 or 7 wins on the alpha band of the photo tile (seed 6: the
band of most seeds is mode 5 throughout)."""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)
TILES = ("photo", "photo2", "ragged", "odd", "ties")
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
    else:
        img = _ties()
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


def _modes(payload):
    """mode of every block: the position of the lowest set bit of its first byte"""
    out = []
    for blk in payload.reshape(-1, 16):
        v = int(blk[0]) | 256
        out.append((v & -v).bit_length() - 1)
    return out


def test_tile_shapes():
    assert _image("photo", "u8").shape == (64, 64, 4) and _image("photo2", "u8").shape == (64, 64, 4)
    assert _image("ragged", "u8").shape == (22, 30, 4) and _image("odd", "u8").shape == (10, 18, 4)
    t = _image("ties", "u8")
    assert t.shape == (16, 16, 4)
    for by in range(4):
        for bx in range(4):
            blk = t[4*by:4*by + 4, 4*bx:4*bx + 4]
            assert (blk == blk[0, 0]).all()
    band = _image("photo", "u8")[32:40, :, 3]
    assert (band < 255).any() and (_image("photo", "u8")[:32, :, 3] == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, ptype, quality, srgb):
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    params = make_params(Format.BC7, Type.UNorm, quality, **kw)
    modes = {}
    for tile in TILES:
        img, ref = _image(tile, ptype), _ref(tile, ptype, quality, srgb)
        got = gpu_ctx.encode([img], params)[0]      # a call of its own: surfaces of one call share a launch
        assert got.size == ref.size == ((img.shape[0] + 3)//4)*((img.shape[1] + 3)//4)*16
        bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
        assert bad.size == 0, "%s: blocks %s differ" % (tile, bad)
        modes[tile] = _modes(got)
    if quality == 2 and not srgb:
        # every mode of Normal's first pass wins somewhere, the two-plane or the alpha-partition mode on the alpha band
        # (block rows 8 and 9 of the photo tile)
        hist = collections.Counter(modes["photo"] + modes["photo2"])
        for mode in (1, 3, 5, 6):
            assert hist[mode] >= 1, sorted(hist.items())
        band = modes["photo"][8*16:10*16]
        assert {4, 7} & set(band), sorted(collections.Counter(band).items())
