"""GPU parity of BC7 after the thirteenth step of DESIGN.md section 4.1: the covariance terms n q - s s by one fused
multiply-add on exact floats, and a fit's weights stored into its candidate's column by and / or on the weight words the
fits share, every winning fit at once (the p-bit word keeps its read-modify-write, one fit at a time).  Both are exact, so every payload (through the C-ABI: Context.encode) must equal the CPU
oracle's byte for byte.  The host side of the identities is tests/test_bc7_gather_trims.py.  (The step's two other
items, 1/n without a table read and the tables read through a uniform base, passed these same cases and were dropped
on their timings: profiles/gather_trims_bc7_ab.txt.)

Tiles
  photo    64 x 64, synth.photo: 256 blocks, one whole workgroup's worth of pairs and more than one workgroup.
  ragged   52 x 36, 13 x 9 blocks: an odd count per row, so the last block of every row runs unpaired, and 117 blocks
           fill no whole workgroup.  Seeded noise, two-region blocks, ramps, half of the noise blocks opaque.
  opaque   32 x 32 of synth.photo with alpha forced to 255: every block takes the three-channel forms (A4 = false).
  band     32 x 32 of synth.photo, alpha 255 outside a band of block rows 2..5 where it ramps: opaque blocks and blocks
           with alpha meet in one wave.
  flat2    32 x 32: flat blocks (n q = s s in every covariance term: exact zeros), blocks of two colours split along a
           row or a column, with and without alpha.
  planted  64 x 32, 128 blocks: block p < 64 holds two colours (with a little grain) laid out as two-subset partition
           p, block 64 + p three colours laid out as three-subset partition p; every second two-subset block carries a
           different alpha per subset.  Phase 1 scores every partition of both tables on every block and the planted
           ones are fitted; their subsets have every size the tables hold (2..8 and 10..13 texels).
Levels 0..4 on photo, ragged, opaque, band and flat2; levels 1, 2 and 3 on planted.  Both metrics, RGBA8 and RGBA32F."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")
BC7 = int(Format.BC7)
TILES = ("photo", "ragged", "opaque", "band", "flat2", "planted")
CASES = [(q, s) for q in range(5) for s in (False, True)]


@functools.lru_cache(maxsize=None)
def _table(name):
    """the 64 words of CF_BC7_PART2_INIT / CF_BC7_PART3_INIT of csrc/bc7_cand.h"""
    text = open(os.path.join(CSRC, "bc7_cand.h")).read()
    body = text[text.index("#define " + name):]
    body = body[:body.index("}")]
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-fA-F]+", body)]
    assert len(words) == 64
    return words


def _subset_of(ns, part, t):
    if ns == 2:
        return (_table("CF_BC7_PART2_INIT")[part] >> t) & 1
    return (_table("CF_BC7_PART3_INIT")[part] >> (2*t)) & 3


def subset_sizes():
    """sizes of the subsets of all 64 + 64 partitions"""
    sizes = set()
    for ns in (2, 3):
        for p in range(64):
            sb = [_subset_of(ns, p, t) for t in range(16)]
            sizes.update(sb.count(k) for k in range(ns))
    return sizes


def _ragged():
    r = np.random.default_rng(131)
    h, w = 36, 52
    img = r.integers(0, 256, (h, w, 4)).astype(np.uint8)
    ramp = np.array([12, 90, 170, 240])
    for by in range(h//4):
        for bx in range(w//4):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            kind = (by*(w//4) + bx) % 5
            if kind == 1:          # two flat regions with a little grain, split along a diagonal
                ca, cb = r.integers(0, 256, 4), r.integers(0, 256, 4)
                for y in range(4):
                    for x in range(4):
                        blk[y, x] = np.clip((ca if x + y < 4 else cb) + r.integers(-2, 3, 4), 0, 255)
            elif kind == 2:        # one line through colour space, all four channels
                for c in range(4):
                    blk[:, :, c] = (ramp if c % 2 else ramp[::-1])[None, :] + np.arange(4)[:, None]
            elif kind == 3:        # a colour channel runs along y, the others and alpha along x
                for c in range(4):
                    blk[:, :, c] = ramp[None, :] + 3*c
                blk[:, :, (by + bx) % 3] = (255 - ramp)[:, None]
            if kind in (0, 4) and bx % 2:
                blk[:, :, 3] = 255
    return img


def _opaque():
    img = synth.photo(32, 32, seed=7).copy()
    img[:, :, 3] = 255
    return img


def _band():
    img = synth.photo(32, 32, seed=8).copy()
    img[:, :, 3] = 255
    img[8:24, :, 3] = np.linspace(20, 250, 16).astype(np.uint8)[:, None]
    return img


def _flat2():
    r = np.random.default_rng(132)
    img = np.zeros((32, 32, 4), np.uint8)
    for by in range(8):
        for bx in range(8):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            ca, cb = r.integers(0, 256, 4), r.integers(0, 256, 4)
            kind = (8*by + bx) % 4
            blk[:, :] = ca
            if kind == 1:
                blk[:, 2:] = cb
            elif kind == 2:
                blk[1:, :] = cb
            elif kind == 3:
                blk[3:, 3:] = cb    # a single texel of the other colour
            if (by + bx) % 2 == 0:
                blk[:, :, 3] = 255
    img[0:4, 0:4] = 0              # all zero, all 255
    img[0:4, 4:8] = 255
    return img


def _planted():
    r = np.random.default_rng(133)
    img = np.zeros((32, 64, 4), np.uint8)
    for b in range(128):
        ns, p = (2, b) if b < 64 else (3, b - 64)
        by, bx = divmod(b, 16)
        blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
        # colours well apart: corners of the colour cube, jittered
        corners = r.permutation(8)[:ns]
        cols = [np.array([(40 if (c >> k) & 1 == 0 else 215) for k in range(3)]) + r.integers(-20, 21, 3) for c in corners]
        alphas = [255]*ns
        if ns == 2 and p % 2:
            alphas = [int(r.integers(20, 120)), int(r.integers(140, 250))]
        for t in range(16):
            sb = _subset_of(ns, p, t)
            blk[t >> 2, t & 3, :3] = np.clip(cols[sb] + r.integers(-2, 3, 3), 0, 255)
            blk[t >> 2, t & 3, 3] = alphas[sb]
    return img


_MAKERS = {"photo": lambda: synth.photo(64, 64, seed=99), "ragged": _ragged, "opaque": _opaque, "band": _band,
           "flat2": _flat2, "planted": _planted}


@functools.lru_cache(maxsize=None)
def _image(tile, ptype):
    img = np.asarray(_MAKERS[tile]())
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


def _levels(tile):
    return (1, 2, 3) if tile == "planted" else (0, 1, 2, 3, 4)


def _modes(payload):
    first = np.asarray(payload).reshape(-1, 16)[:, 0].astype(np.uint32).tolist()
    return [int(b & -b).bit_length() - 1 for b in first]


def _partition(block):
    """(mode, partition) of a 16-byte block of a partitioned mode"""
    v = int.from_bytes(bytes(bytearray(block)), "little")
    mode = (v & -v).bit_length() - 1
    nbits = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}[mode]
    return mode, (v >> (mode + 1)) & ((1 << nbits) - 1)


def test_tile_shapes():
    assert _image("photo", "u8").shape == (64, 64, 4)
    g = _image("ragged", "u8")
    assert g.shape == (36, 52, 4) and (g.shape[1]//4) % 2 == 1 and (g.shape[0]//4)*(g.shape[1]//4) == 117
    assert (_image("opaque", "u8")[:, :, 3] == 255).all()
    b = _image("band", "u8")
    assert (b[:8, :, 3] == 255).all() and (b[8:24, :, 3] < 255).all() and (b[24:, :, 3] == 255).all()
    f = _image("flat2", "u8")
    blocks = [f[4*y:4*y + 4, 4*x:4*x + 4] for y in range(8) for x in range(8)]
    assert sum(bool((k == k[0, 0]).all()) for k in blocks) >= 16
    assert sum(len({tuple(px) for row in k for px in row}) == 2 for k in blocks) >= 40
    assert _image("planted", "u8").shape == (32, 64, 4)


def test_subset_sizes_the_tables_hold():
    """the sizes n of the covariance terms: these and the whole block (16 texels: mode 6, the planes of modes 4 / 5).
    The tables hold no subset of 1, 9, 14 or 15 texels; the planted tile below reaches every size they do hold."""
    assert subset_sizes() == {2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13}


def test_planted_partitions_reach_the_payload():
    """what the GPU assertion on `planted` rests on.  Every block's planted partition is scored and fitted (phase 1
    ranks all 64 + 64 shapes on every block), whichever mode wins in the end; in the oracle's own Normal payload every
    opaque two-subset block is coded by a two-subset mode with exactly its planted partition, and three-subset
    modes win some of the three-colour blocks (their 5-bit endpoints lose most of them to mode 3)."""
    ref = np.asarray(_ref("planted", "u8", 2, False)).reshape(-1, 16)
    modes = _modes(ref)
    for b in range(0, 64, 2):
        assert modes[b] in (1, 3, 7) and _partition(ref[b])[1] == b, (b, modes[b])
    assert any(m in (0, 2) for m in modes[64:])


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, ptype, quality, srgb):
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    params = make_params(Format.BC7, Type.UNorm, quality, **kw)
    for tile in TILES:
        if quality not in _levels(tile):
            continue
        img, ref = _image(tile, ptype), _ref(tile, ptype, quality, srgb)
        got = gpu_ctx.encode([img], params)[0]      # a call of its own: surfaces of one call share a launch
        assert got.size == ref.size == ((img.shape[0] + 3)//4)*((img.shape[1] + 3)//4)*16
        bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
        assert bad.size == 0, "%s: blocks %s differ" % (tile, bad)
