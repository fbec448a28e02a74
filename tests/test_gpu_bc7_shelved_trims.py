"""GPU parity of BC7 after the twelfth step of DESIGN.md section 4.1: mode 6's half exchange once per row under the
execution mask, part B's projection extremes by three-operand minimum / maximum over texels masked to a quiet NaN, the
fit's error from the sum of the masked keys, the block packed from a table per (candidate shape, field slot), the refit
sums unrolled.  Every item is exact, so every payload must equal the CPU oracle's byte for
byte, at levels 0..4, with both metrics, from an RGBA8 and from an RGBA32F source.  The host side of the identities is
tests/test_bc7_shelved_trims.py.

Tiles: those of test_gpu_bc7_search_bias.py (imported: images and oracle payloads are shared with that module) and
  ragged   36 x 20 texels, 9 x 5 blocks: an odd count per row, so the last block of every row runs unpaired (one block in a
           wave that holds two), and 45 blocks fill no whole workgroup.  Seeded noise, two-region blocks, blocks on one
           line through colour space and blocks whose red (green, blue) channel runs across the other three, which
           vary together with alpha: the shape modes 4 / 5 code with a rotation.
  zeros    16 x 16: blocks that are flat, flat in one region and noisy in the other (a two-subset shape with one
           all-equal subset), or a pure ramp of one channel along x or y with the others constant: the projections on the
           axis are then exactly 0 for a flat subset (every texel equals the mean) and symmetric about 0 for a ramp, so
           zeros of both signs and ties meet the minimum / maximum.  Half of the blocks carry alpha.
On the CPU: the oracle's Normal payloads of the two tiles hold mode-6 blocks, two-subset blocks and mode-5 blocks with a
rotation, and `ragged` ends its rows on an unpaired block."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_bc7_search_bias as B
from cuttlefish_amd import ColorSpace, Format, Type, make_params

BC7 = int(Format.BC7)
NEW_TILES = ("ragged", "zeros")
TILES = B.TILES + NEW_TILES
CASES = B.CASES


def _ragged():
    r = np.random.default_rng(57)
    h, w = 20, 36
    img = r.integers(0, 256, (h, w, 4)).astype(np.uint8)
    ramp = np.array([16, 84, 160, 236])
    for by in range(h//4):
        for bx in range(w//4):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            kind = (by*(w//4) + bx) % 6
            if kind == 1:          # two flat regions with a little grain, split along a diagonal
                ca, cb = r.integers(0, 256, 4), r.integers(0, 256, 4)
                for y in range(4):
                    for x in range(4):
                        blk[y, x] = np.clip((ca if x + y < 4 else cb) + r.integers(-2, 3, 4), 0, 255)
            elif kind == 2:        # one line through colour space, all four channels: mode 6's shape
                for c in range(4):
                    blk[:, :, c] = (ramp if c % 2 else ramp[::-1])[None, :] + np.arange(4)[:, None]
            elif kind >= 3:        # colour kind - 3 runs along y, the other two and alpha run together along x
                ch = kind - 3
                for c in range(4):
                    blk[:, :, c] = ramp[None, :] + 3*c
                blk[:, :, ch] = (255 - ramp)[:, None]
            if kind == 0 and bx % 2:
                blk[:, :, 3] = 255
    return img


def _zeros():
    r = np.random.default_rng(58)
    img = np.zeros((16, 16, 4), np.uint8)
    for by in range(4):
        for bx in range(4):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            kind = (4*by + bx) % 4
            col = r.integers(0, 256, 4)
            blk[:, :] = col
            if kind == 1:          # flat on one side of a diagonal, seeded noise on the other
                for y in range(4):
                    for x in range(4):
                        if x + y >= 4:
                            blk[y, x] = r.integers(0, 256, 4)
            elif kind == 2:        # one channel ramps along x, symmetric about its mean; the others are constant
                blk[:, :, (by + bx) % 3] = np.array([98, 118, 138, 158])[None, :]
            elif kind == 3:        # one channel ramps along y from 0
                blk[:, :, (by + bx) % 3] = np.array([0, 85, 170, 255])[:, None]
            # half of the blocks carry alpha, the others are opaque
            if (by + bx) % 2 == 0:
                blk[:, :, 3] = 255
            elif kind == 0:
                blk[:, :, 3] = 77
    return img


@functools.lru_cache(maxsize=None)
def _image(tile, ptype):
    if tile not in NEW_TILES:
        return B._image(tile, ptype)
    img = _ragged() if tile == "ragged" else _zeros()
    if ptype == "f32":
        img = (img.astype(np.float64)/255.0).astype(np.float32)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(tile, ptype, quality, srgb):
    if tile not in NEW_TILES:
        return B._ref(tile, ptype, quality, srgb)
    ref = O.encode(_image(tile, ptype), BC7, quality=quality, threads=4, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return ref


def _first_bytes(payload):
    return np.asarray(payload).reshape(-1, 16)[:, 0].astype(np.uint32).tolist()


def _kinds(payloads):
    """(mode-6 blocks, two-subset blocks, mode-5 blocks with a rotation) over the payloads"""
    m6 = two = rot5 = 0
    for p in payloads:
        for b in _first_bytes(p):
            mode = int(b & -b).bit_length() - 1
            m6 += mode == 6
            two += mode in (1, 3, 7)
            rot5 += mode == 5 and (b >> 6) != 0     # mode 5: bit 5 set, the rotation in bits 6..7
    return m6, two, rot5


def test_tile_shapes():
    g, z = _image("ragged", "u8"), _image("zeros", "u8")
    assert g.shape == (20, 36, 4) and z.shape == (16, 16, 4)
    # 9 blocks per row: every row ends on a block without a partner, and 45 blocks fill no whole workgroup
    assert (g.shape[1]//4) % 2 == 1 and g.shape[1] % 4 == 0 and g.shape[0] % 4 == 0
    assert _ref("ragged", "u8", 2, False).size == 9*5*16
    blocks = [z[4*by:4*by + 4, 4*bx:4*bx + 4] for by in range(4) for bx in range(4)]
    flat = [bool((b == b[0, 0]).all()) for b in blocks]
    assert sum(flat) == 4
    assert sum(bool((b[:, :, 3] == 255).all()) for b in blocks) == 8
    # flat in one subset only: the texels above the diagonal are one colour, the others are not
    assert sum(1 for b in blocks if not (b == b[0, 0]).all() and all((b[y, x] == b[0, 0]).all() for y in range(4) for x in range(4) if x + y < 4)
               and len({tuple(b[y, x]) for y in range(4) for x in range(4) if x + y >= 4}) > 2) == 4
    # a pure axis-aligned ramp: one channel varies, along one direction
    ramps = 0
    for b in blocks:
        var = [c for c in range(4) if len(np.unique(b[:, :, c])) > 1]
        if len(var) == 1 and ((b[:, :, var[0]] == b[:1, :, var[0]]).all() or (b[:, :, var[0]] == b[:, :1, var[0]]).all()):
            ramps += 1
    assert ramps == 8


def test_new_tiles_ask_for_every_kind_of_fit():
    """what the GPU assertion below rests on: the oracle's own Normal payloads of the two tiles hold mode-6 blocks,
    two-subset blocks and mode-5 blocks with a non-zero rotation"""
    kinds = _kinds([_ref(t, "u8", 2, False) for t in NEW_TILES])
    assert all(k > 0 for k in kinds), kinds


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, ptype, quality, srgb):
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    params = make_params(Format.BC7, Type.UNorm, quality, **kw)
    normal = []
    for tile in TILES:
        img, ref = _image(tile, ptype), _ref(tile, ptype, quality, srgb)
        got = gpu_ctx.encode([img], params)[0]      # a call of its own: surfaces of one call share a launch
        assert got.size == ref.size == ((img.shape[0] + 3)//4)*((img.shape[1] + 3)//4)*16
        bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
        assert bad.size == 0, "%s: blocks %s differ" % (tile, bad)
        if tile in NEW_TILES:
            normal.append(np.asarray(got))
    if quality == 2 and not srgb:
        assert all(k > 0 for k in _kinds(normal)), _kinds(normal)
