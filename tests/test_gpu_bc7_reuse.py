"""GPU parity of BC7's reuse paths: the starts trip reads each fit's geometry (axis, mean, projection
extremes, pp_sum) from the stream-trip lane that fitted it when every lane of the wave finds its fit there,
and falls back to the full fit otherwise; the perturbation pass walks 4 palette entries instead of 8 when no
fit of the wave has more.  Both are exact rewrites, so every payload must equal the CPU oracle's."""
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


def _mixed(width, height, seed):
    """Smooth photo content (blocks solved in the first pass), noisy blocks (they walk the second pass:
    their best first-pass error is >= 48), flat and two-tone blocks, and an alpha band -- so that the pairs
    of one wave mix halves that did and did not walk the second pass."""
    rng = np.random.default_rng(seed)
    img = synth.photo2(width, height, seed=seed).copy()
    img[..., 3] = 255
    bw = width // 4
    for by in range(height // 4):
        for bx in range(bw):
            k = (by * 7 + bx * 3 + seed) % 6
            blk = img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            if k == 0:
                blk[..., :3] = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
            elif k == 1:
                blk[..., :3] = rng.integers(0, 256, 3, dtype=np.uint8)
            elif k == 2:
                two = rng.integers(0, 256, (2, 3), dtype=np.uint8)
                sel = (np.arange(16).reshape(4, 4) * 5 + bx) % 3 == 0
                blk[..., :3] = np.where(sel[..., None], two[0], two[1])
    img[height // 2:height // 2 + 4, :, 3] = np.linspace(0, 255, width).astype(np.uint8)
    return img


def _check(ctx, img, quality, srgb=False):
    ref = O.encode(img, BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    got = _gpu(ctx, img, quality, color_space=ColorSpace.sRGB) if srgb else _gpu(ctx, img, quality)
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "blocks differ: %s" % bad[:10]
    return ref


@pytest.mark.parametrize("quality", [0, 1, 2, 3, 4])
def test_mixed_tile_all_levels(gpu_ctx, quality):
    # 37 block columns: the last block of every strip row runs unpaired, the last 2 texel columns are ragged
    _check(gpu_ctx, _mixed(146, 48, seed=3 + quality), quality)


@pytest.mark.parametrize("quality", [2, 3, 4])
def test_mixed_tile_perceptual(gpu_ctx, quality):
    _check(gpu_ctx, _mixed(146, 32, seed=11 + quality), quality, srgb=True)


def test_alpha_tile(gpu_ctx):
    img = synth.photo(130, 36, seed=21)
    _check(gpu_ctx, img, 2)


@pytest.mark.parametrize("quality", [2, 3])
def test_narrow_palette_taken(gpu_ctx, quality):
    """Smooth two-channel ramps with a little noise end in 2-bit modes (5 / 3 / 7) with a nonzero error:
    whole pairs of blocks then perturb with the 4-entry selector search."""
    rng = np.random.default_rng(5 + quality)
    y, x = np.mgrid[0:64, 0:128]
    img = np.empty((64, 128, 4), np.uint8)
    img[..., 0] = (x * 2 + rng.integers(0, 3, x.shape)).clip(0, 255)
    img[..., 1] = (y * 3 + rng.integers(0, 3, x.shape)).clip(0, 255)
    img[..., 2] = 40
    img[..., 3] = 255
    ref = _check(gpu_ctx, img, quality)
    m = _modes(ref).reshape(-1, 2)
    narrow = np.isin(m, (3, 5, 7)).all(axis=1)
    assert narrow.mean() > 0.5, np.bincount(_modes(ref), minlength=8)


def test_narrow_palette_not_taken(gpu_ctx):
    """Noise ends in modes with 3- and 4-bit indices (1, 6, 0): the 8-entry search."""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (32, 64, 4), dtype=np.uint8)
    img[..., 3] = 255
    ref = _check(gpu_ctx, img, 2)
    assert np.isin(_modes(ref), (0, 1, 6)).any()
