"""GPU parity of BC7's per-level kernel instances: every quality level 0..4 has an instance of its own whose search
budget (refit rounds, list length, perturbation rounds, move sets, lane layout) is a compile-time constant, so each
level is checked on its own -- linear and sRGB (perceptual) metric, RGBA8 and RGBA32F sources -- against the CPU
oracle, block by block.

Shapes, for the dispatch and pairing paths (two neighbouring blocks share a wave up to Normal):
  64 x 16  a full workgroup per block row, every wave paired
  20 x 12  five blocks per row: wave 1 takes a single unpaired block
  68 x 8   a second workgroup that holds one block
  one batched call of a 20 x 12 RGBA8, an 8 x 8 RGBA32F and a 4 x 4 RGBA32F surface

All of them are crops of one mixed tile: photo content, per-block noise, flat blocks (odd values: exact in mode 6),
two-tone blocks, blocks whose one channel follows a gradient of its own (modes 4 / 5), and an alpha ramp over block
columns 3..12 of block row 1 -- it starts at an odd column, so the pair (2, 3) has an opaque and an alpha-carrying
half.  What the tile has to exercise is a condition on the oracle's payload of the 64 x 16 crop alone (the
*_exercise tests, no GPU)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)
TILE_W, TILE_H = 68, 16
A_ROW, A_FIRST, A_LAST = 1, 3, 12          # the alpha ramp: block row, first and last block column
SEED = 4
LEVELS = [0, 1, 2, 3, 4]
# name -> (x0, y0, width, height) of the crop
SHAPES = {"w64": (0, 0, 64, 16), "w20": (0, 0, 20, 12), "w68": (0, 4, 68, 8)}
BATCH = (("u8", (0, 0, 20, 12)), ("f32", (8, 4, 8, 8)), ("f32", (12, 4, 4, 4)))


@functools.lru_cache(maxsize=None)
def _mixed(seed):
    rng = np.random.default_rng(seed)
    img = synth.photo2(TILE_W, TILE_H, seed=seed).copy()
    img[..., 3] = 255
    yy, xx = np.mgrid[0:4, 0:4]
    for by in range(TILE_H // 4):
        for bx in range(TILE_W // 4):
            k = (by * 5 + bx * 3 + seed) % 8
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            if k == 0:
                blk[..., :3] = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
            elif k == 1:
                blk[..., :3] = rng.integers(0, 128, 3, dtype=np.uint8) * 2 + 1
            elif k == 2:
                two = rng.integers(0, 256, (2, 3), dtype=np.uint8)
                sel = (np.arange(16).reshape(4, 4) * 7 + bx) % 3 == 0
                blk[..., :3] = np.where(sel[..., None], two[0], two[1])
            elif k == 3:
                c = int(rng.integers(0, 3))
                g = (rng.integers(20, 60) + xx * rng.integers(8, 40) + rng.integers(-2, 3, (4, 4))).clip(0, 255)
                s = (rng.integers(20, 60) + yy * rng.integers(8, 50) + rng.integers(-2, 3, (4, 4))).clip(0, 255)
                for ch in range(3):
                    blk[..., ch] = s if ch == c else g
    ramp = np.linspace(0, 255, 4 * (A_LAST - A_FIRST + 1)).astype(np.uint8)
    img[4 * A_ROW:4 * A_ROW + 4, 4 * A_FIRST:4 * A_LAST + 4, 3] = ramp
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(crop, ptype, quality, srgb):
    """Source and oracle payload of one case: computed once, shared by the exercise and the parity tests"""
    x0, y0, w, h = crop
    img = np.ascontiguousarray(_mixed(SEED)[y0:y0 + h, x0:x0 + w])
    if ptype == "f32":
        img = (img.astype(np.float64) / 255.0).astype(np.float32)
    ref = O.encode(img, BC7, quality=quality, threads=4, color_space=1 if srgb else 0)
    img.setflags(write=False)
    ref.setflags(write=False)
    return img, ref


def _modes(payload):
    """BC7 mode of every block: the position of the lowest set bit of its first byte"""
    b0 = payload.reshape(-1, 16)[:, 0].astype(np.int64)
    return np.array([(int(v) & -int(v)).bit_length() - 1 for v in b0])


def _blocks(img):
    """(h, w, 4) -> (blocks in payload order, 64): the 16 texels of every block"""
    h, w = img.shape[:2]
    return img.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 64)


def _params(quality, srgb):
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    return make_params(Format.BC7, Type.UNorm, quality, **kw)


# ---- what the tile exercises: conditions on the oracle's output alone (no GPU) ----

def test_alpha_ramp_splits_a_pair():
    """Blocks 2 and 3 of block row 1 share a wave: one opaque, one with alpha (in the 20-wide crop too)"""
    a = (_blocks(_mixed(SEED)[:, :64])[:, 3::4] != 255).any(axis=1).reshape(4, 16)
    assert not a[A_ROW, 2] and a[A_ROW, 3] and a[A_ROW, A_LAST] and not a[A_ROW, A_LAST + 1]
    assert SHAPES["w20"][2] // 4 > 3 and SHAPES["w20"][3] // 4 > A_ROW


@pytest.mark.parametrize("srgb", [False, True])
def test_normal_exercise(srgb):
    """Normal: every mode of the first pass; both kinds of second pass (three subsets for an opaque half, mode 4 for
    one with alpha); a block solved exactly (its search ends early); a pair of which one half alone walks the second pass"""
    img, ref = _ref(SHAPES["w64"], "u8", 2, srgb)
    m = _modes(ref)
    for mode in (1, 3, 5, 6, 7):
        assert (m == mode).any(), np.bincount(m, minlength=8)
    assert np.isin(m, (0, 2)).any() and (m == 4).any(), np.bincount(m, minlength=8)
    dec = O.decode(ref, BC7, img.shape[1], img.shape[0])
    assert (_blocks(dec) == _blocks(img)).all(axis=1).any(), "no zero-error block"
    second = np.isin(m, (0, 2, 4))
    assert (second[0::2] != second[1::2]).any(), "no pair with exactly one three-subset / mode-4 half"


@pytest.mark.parametrize("quality", [3, 4])
def test_high_exercise(quality):
    """High, Highest: mode 4 on an opaque block (linear metric: the perceptual one admits no channel rotation)"""
    img, ref = _ref(SHAPES["w64"], "u8", quality, False)
    opaque = (_blocks(img)[:, 3::4] == 255).all(axis=1)
    assert ((_modes(ref) == 4) & opaque).any(), np.bincount(_modes(ref), minlength=8)


@pytest.mark.parametrize("srgb", [False, True])
def test_lowest_exercise(srgb):
    """Lowest: mode 6, and mode 5 on a block with alpha"""
    img, ref = _ref(SHAPES["w64"], "u8", 0, srgb)
    m = _modes(ref)
    alpha = (_blocks(img)[:, 3::4] != 255).any(axis=1)
    assert (m == 6).any() and ((m == 5) & alpha).any(), np.bincount(m, minlength=8)


# ---- parity ----

def _assert_same(ref, got, what):
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "%s: blocks differ: %s" % (what, bad[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quality", LEVELS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_level_instance(gpu_ctx, shape, quality, srgb, ptype):
    img, ref = _ref(SHAPES[shape], ptype, quality, srgb)
    got = gpu_ctx.encode([img], _params(quality, srgb))[0]
    _assert_same(ref, got, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("quality", LEVELS)
def test_level_instance_batched(gpu_ctx, quality, srgb):
    """Three surfaces of two source types in one call: one batched launch per run of a type"""
    cases = [_ref(crop, ptype, quality, srgb) for ptype, crop in BATCH]
    gots = gpu_ctx.encode([img for img, _ in cases], _params(quality, srgb))
    assert len(gots) == len(cases)
    for i, ((_, ref), got) in enumerate(zip(cases, gots)):
        _assert_same(ref, got, "surface %d" % i)
