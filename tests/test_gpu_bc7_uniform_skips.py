"""GPU parity of BC7's exact rewrites that issue fewer instructions: phase 1 sums the statistics of the non-zero
subsets in one pass over the rows and takes subset 0 as the block's table entry minus them, three-subset masks
come from bit operations on the partition word, the perturbation pass reads pp_sum from the fit-geometry cache
when every lane finds its fit there and dequantises without p-bits when no fit of the wave has any, and the
unit-weight builds rank candidates by one 32-bit (error << 9 | id) key.  Every payload must equal the CPU oracle's."""
import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

pytestmark = pytest.mark.gpu
BC7 = int(Format.BC7)


def _gpu(ctx, img, quality, **kw):
    return ctx.encode([img], make_params(Format.BC7, Type.UNorm, quality, **kw))[0]


def _modes(payload):
    """BC7 mode of every block: the position of the lowest set bit of its first byte"""
    b0 = payload.reshape(-1, 16)[:, 0].astype(np.int64)
    return np.array([(int(v) & -int(v)).bit_length() - 1 for v in b0])


def _check(ctx, img, quality, srgb=False):
    ref = O.encode(img, BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    got = _gpu(ctx, img, quality, color_space=ColorSpace.sRGB) if srgb else _gpu(ctx, img, quality)
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "blocks differ: %s" % bad[:10]
    return ref


def _ramps(width, height, seed):
    """Smooth ramps in two channels with +-2 noise, opaque: the winners are mostly mode 5"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    img = np.empty((height, width, 4), np.uint8)
    img[..., 0] = (x + 40 + rng.integers(-2, 3, x.shape)).clip(0, 255)
    img[..., 1] = (2 * y + 60 + rng.integers(-2, 3, x.shape)).clip(0, 255)
    img[..., 2] = 40
    img[..., 3] = 255
    return img


def _noise(width, height, seed):
    img = np.random.default_rng(seed).integers(0, 256, (height, width, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def _mixed(width, height, seed):
    """Photo content, noise, flat and two-tone blocks and an alpha band in one tile"""
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
    img[height // 2:height // 2 + 4, :, 3] = np.linspace(0, 255, width).astype(np.uint8)
    return img


@pytest.mark.parametrize("quality", [2, 3])
def test_ramps_without_p_bits(gpu_ctx, quality):
    """Mode 5 wins most blocks, so whole perturbation passes have no fit with p-bits."""
    ref = _check(gpu_ctx, _ramps(128, 64, seed=31 + quality), quality)
    m = _modes(ref)
    assert (m == 5).mean() > 0.5, np.bincount(m, minlength=8)


def test_alternating_block_columns(gpu_ctx):
    """Noise along one colour line (it ends in the p-bit modes 1 / 3 / 6) in the even block columns and smooth
    ramps in the odd ones: a pair mixes a half with p-bits and one without; 37 block columns, so the last block
    of a row runs unpaired."""
    rng = np.random.default_rng(42)
    img = _ramps(148, 32, seed=41)
    noise = img.copy()
    line = rng.integers(-100, 101, (32, 148, 1)) * np.array([1.0, 0.7, -0.5])
    noise[..., :3] = (np.array([120, 100, 140]) + line + rng.integers(-6, 7, (32, 148, 3))).clip(0, 255)
    cols = (np.arange(148) // 4) % 2 == 0
    img[:, cols] = noise[:, cols]
    ref = _check(gpu_ctx, img, 2)
    m = _modes(ref).reshape(8, 37)
    assert np.isin(m[:, 0::2], (1, 3, 6)).mean() > 0.5, np.bincount(m.ravel(), minlength=8)
    assert (m[:, 1::2] == 5).any()


@pytest.mark.parametrize("quality", [2, 3, 4])
def test_noisy_blocks_second_pass(gpu_ctx, quality):
    """Noisy opaque blocks walk the second pass: three-subset masks, and at Normal the subsets' complement."""
    ref = _check(gpu_ctx, _noise(64, 32, seed=50 + quality), quality)
    assert np.isin(_modes(ref), (0, 2)).any(), np.bincount(_modes(ref), minlength=8)


def test_alpha_row_in_opaque_image(gpu_ctx):
    """One block row carries an alpha ramp that saturates inside block 4: blocks 0..4 of that row have alpha,
    the rest are opaque, so the pair (4, 5) has one half of each kind."""
    img = synth.photo2(72, 12, seed=61).copy()
    img[..., 3] = 255
    img[4:8, :, 3] = np.minimum(255, np.arange(72) * 255 // 19).astype(np.uint8)
    a = img[4:8, :, 3].reshape(4, 18, 4)
    assert (a[:, 4] != 255).any() and (a[:, 5:] == 255).all()
    for quality in (2, 3):
        _check(gpu_ctx, img, quality)


def test_translucent(gpu_ctx):
    img = synth.photo2(32, 16, seed=62).copy()
    img[..., 3] = np.random.default_rng(63).integers(0, 255, (16, 32), dtype=np.uint8)
    for quality in (2, 3):
        _check(gpu_ctx, img, quality)


@pytest.mark.parametrize("shape", [(4, 4), (20, 8), (17, 9)])
def test_shapes(gpu_ctx, shape):
    """One block; five block columns, the fifth unpaired; ragged edges."""
    w, h = shape
    img = _mixed(max(w, 8), max(h, 8), seed=71)[:h, :w].copy()
    for quality in (2, 3):
        _check(gpu_ctx, img, quality)


def test_extreme_errors(gpu_ctx):
    """Texels of random 0 / 255 in all four channels: the largest errors a block can have, at the bound the
    32-bit candidate key is built on."""
    img = (np.random.default_rng(81).integers(0, 2, (16, 64, 4)) * 255).astype(np.uint8)
    for quality in (2, 3, 4):
        _check(gpu_ctx, img, quality)


def test_flat_blocks(gpu_ctx):
    """Flat blocks have zero error and leave the search early."""
    rng = np.random.default_rng(82)
    img = np.repeat(np.repeat(rng.integers(0, 256, (4, 16, 4), dtype=np.uint8), 4, axis=0), 4, axis=1)
    img[:, :32, 3] = 255
    for quality in (2, 3, 4):
        _check(gpu_ctx, img, quality)


@pytest.mark.parametrize("quality", [0, 1, 2, 3, 4])
def test_mixed_tile_all_levels(gpu_ctx, quality):
    _check(gpu_ctx, _mixed(148, 48, seed=90 + quality), quality)


@pytest.mark.parametrize("quality", [2, 3])
def test_mixed_tile_perceptual(gpu_ctx, quality):
    _check(gpu_ctx, _mixed(148, 32, seed=95 + quality), quality, srgb=True)
