"""GPU parity of BC7 with the unit-weight selector search issued without the C operand of its matrix-pipe instruction:
the texel's own term 128 sum_c a_c leaves every key and is taken off the fit's constant pp_sum once, from the per-block
table word (whole-block fits) or the fit's own subset sums (partition fits) -- DESIGN.md section 4.1, eleventh step;
search_pp_fold, search_bias_part and lohi_pack in csrc/bc7_packed.h, on the CPU in tests/test_bc7_search_bias.py.
Every payload must equal the CPU oracle's byte for byte, at levels 0..4, with both metrics (the perceptual instances keep
their code and are covered as the untouched half), from an RGBA8 and from an RGBA32F source.

Tiles: the seven of test_gpu_bc7_mfma_dots.py (their images and oracle payloads are shared with that module) and
  dark     16 x 16: every channel in 0..3 (seeded noise, two-region, ramp and diagonal blocks: _tile), half of the blocks
           opaque, the others with alpha 0..3: 256 sum a exceeds sum p^2 by the widest relative margin, the folded constant
           lies below zero in every fit
  bright   16 x 16: every channel in 252..255 (the same patterns), opaque blocks and blocks with alpha (252..255, at least
           one texel below 255) alternating along x, so that both kinds share a wave pair: the largest bias, on whole-block
           and partition fits of both kinds (channel set 7 with the constant alpha added, channel set 15)
Over these two tiles the oracle's Normal payloads hold two-subset blocks (modes 1, 3 or 7) and mode-6 blocks: checked on the
CPU below, and on the GPU's payloads.  The oracle's payloads are computed once per case and shared."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_bc7_mfma_dots as D
from cuttlefish_amd import ColorSpace, Format, Type, make_params

BC7 = int(Format.BC7)
NEW_TILES = ("dark", "bright")
TILES = D.TILES + NEW_TILES
CASES = D.CASES


def _tile(base, opaque_of):
    """16 x 16 with every channel in base .. base + 3.  Pairs of neighbouring blocks share a pattern, one of them opaque:
    seeded noise; two flat regions split along a diagonal (a two-subset shape); all four channels ramping along x
    together, each up or down; all four following one diagonal ramp (one line through colour space: mode 6's shape)."""
    r = np.random.default_rng(31)
    img = (base + r.integers(0, 4, (16, 16, 4))).astype(np.uint8)
    diag = np.array([[0, 1, 1, 2], [1, 1, 2, 2], [1, 2, 2, 3], [2, 2, 3, 3]])
    for by in range(4):
        for bx in range(4):
            blk = img[4*by:4*by + 4, 4*bx:4*bx + 4]
            kind = ((4*by + bx)//2) % 4
            if kind == 1:
                ca, cb = base + r.integers(0, 4, 4), base + r.integers(0, 4, 4)
                for y in range(4):
                    for x in range(4):
                        blk[y, x] = ca if x + y < 4 else cb
            elif kind == 2:
                for c in range(4):
                    ramp = np.arange(4) if r.integers(0, 2) else np.arange(4)[::-1]
                    blk[:, :, c] = base + ramp[None, :]
            elif kind == 3:
                for c in range(4):
                    blk[:, :, c] = base + diag
            if opaque_of(by, bx):
                blk[:, :, 3] = 255
            elif base == 252:
                blk[(bx + by) % 4, by, 3] = 252
    return img


def _dark():
    return _tile(0, lambda by, bx: (by + bx) % 2 == 0)


def _bright():
    return _tile(252, lambda by, bx: bx % 2 == 0)


@functools.lru_cache(maxsize=None)
def _image(tile, ptype):
    if tile not in NEW_TILES:
        return D._image(tile, ptype)
    img = _dark() if tile == "dark" else _bright()
    if ptype == "f32":
        img = (img.astype(np.float64)/255.0).astype(np.float32)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(tile, ptype, quality, srgb):
    if tile not in NEW_TILES:
        return D._ref(tile, ptype, quality, srgb)
    ref = O.encode(_image(tile, ptype), BC7, quality=quality, threads=4, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return ref


def _modes(payload):
    """mode of every block: the position of the lowest set bit of its first byte"""
    first = np.asarray(payload).reshape(-1, 16)[:, 0].astype(np.uint32)
    return [int(b & -b).bit_length() - 1 for b in first.tolist()]


def _has_both_kinds(payloads):
    modes = [m for p in payloads for m in _modes(p)]
    return any(m in (1, 3, 7) for m in modes) and any(m == 6 for m in modes)


def test_tile_shapes():
    d, b = _image("dark", "u8"), _image("bright", "u8")
    assert d.shape == b.shape == (16, 16, 4)
    assert set(np.unique(d[:, :, :3])) == {0, 1, 2, 3} and set(np.unique(b)) == {252, 253, 254, 255}
    opaque = [(d[4*by:4*by + 4, 4*bx:4*bx + 4, 3] == 255).all() for by in range(4) for bx in range(4)]
    assert sum(opaque) == 8
    assert all(int(d[4*by:4*by + 4, 4*bx:4*bx + 4, 3].max()) <= 3 for by in range(4) for bx in range(4) if (by + bx) % 2)
    for by in range(4):
        for bx in range(4):
            a = b[4*by:4*by + 4, 4*bx:4*bx + 4, 3]
            assert (a == 255).all() if bx % 2 == 0 else (a < 255).any(), (by, bx)


def test_new_tiles_ask_for_partition_and_mode6_fits():
    """what the GPU assertion below rests on: the oracle's own Normal payloads of the two tiles hold both kinds of block"""
    modes = {t: sorted(set(_modes(_ref(t, "u8", 2, False)))) for t in NEW_TILES}
    assert _has_both_kinds([_ref(t, "u8", 2, False) for t in NEW_TILES]), modes


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
        assert _has_both_kinds(normal), [_modes(p) for p in normal]
