"""The numpy twin of alpha bleeding (tests/alpha_bleed_ref.py) against brute force, and the laws of the definition.
No GPU: the kernels are compared with the twin in test_gpu_alpha_bleed.py."""
import numpy as np
import pytest

import alpha_bleed_ref as R

SURFACES = ((40, 48), (21, 37), (64, 64), (33, 100))            # (h, w)
DENSITIES = (0.002, 0.01, 0.05, 0.3)
# the share of texels whose jump-flood seed may be farther than the exact nearest one, over the whole set below: a
# condition of the definition (the trailing step of 1 is what keeps it), not a measurement
ABOVE_EXACT_CAP = 1e-3


def image_of(mask, dtype=np.uint8, seed=0):
    """random colour everywhere, alpha 1 on the mask and 0 off it"""
    rng = np.random.default_rng(seed)
    h, w = mask.shape
    img = np.concatenate([rng.random((h, w, 3)), mask[..., None].astype(np.float64)], -1)
    return np.round(img*255).astype(np.uint8) if dtype == np.uint8 else img.astype(dtype)


def test_jump_flood_against_exact_nearest_seed():
    rng = np.random.default_rng(20261020)
    texels = above = 0
    worst = 0.0
    for h, w in SURFACES:
        for density in DENSITIES:
            for wrap in (False, True):
                for _ in range(4):
                    mask = rng.random((h, w)) < density
                    if not mask.any():                          # a draw without a seed says nothing about the search
                        mask[rng.integers(h), rng.integers(w)] = True
                    words, d2 = R.jump_flood(mask, wrap, wrap)
                    ewords, ed2 = R.exact_nearest(mask, wrap, wrap)
                    assert (words != R.NONE).all(), (h, w, density, wrap)
                    y, x = np.mgrid[0:h, 0:w]
                    assert mask[words >> 16, words & 0xFFFF].all()          # every word names a seed
                    assert np.array_equal(d2, R.dist2(x, y, words, w, h, wrap, wrap))
                    assert (d2 >= ed2).all(), (h, w, density, wrap)
                    same = d2 == ed2
                    assert np.array_equal(words[same] >= ewords[same], np.ones(same.sum(), bool))
                    texels += h*w
                    above += int((~same).sum())
                    if (~same).any():
                        worst = max(worst, float((np.sqrt(d2[~same].astype(np.float64)) - np.sqrt(ed2[~same].astype(np.float64))).max()))
    print("jump flood above exact: %d of %d texels (%.2e), worst excess %.2f texels" % (above, texels, above/texels, worst))
    assert texels == 322976
    assert above <= ABOVE_EXACT_CAP*texels


def test_steps():
    assert R.steps_of(1, 1) == [1]
    assert R.steps_of(2, 1) == [1, 1]
    assert R.steps_of(17, 1) == R.steps_of(1, 17) == R.steps_of(32, 32) == [16, 8, 4, 2, 1, 1]
    assert R.steps_of(33, 100) == [64, 32, 16, 8, 4, 2, 1, 1]
    assert R.steps_of(32768, 3)[0] == 16384 and len(R.steps_of(32768, 3)) == 16


@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
def test_seeds_and_alpha_never_change_and_the_pass_is_idempotent(dtype):
    rng = np.random.default_rng(3)
    mask = rng.random((21, 37)) < 0.1
    img = image_of(mask, dtype, 4)
    for wrap in (False, True, (True, False)):
        out, rec = R.bleed(img, 0.0, wrap)
        assert out.dtype == img.dtype and out[..., 3].tobytes() == img[..., 3].tobytes()
        assert out[mask].tobytes() == img[mask].tobytes()
        assert rec["seeds"] == mask.sum() and rec["filled"] == (~mask).sum() and rec["reserved"] == 0
        # every filled texel holds the bits of a seed's colour
        colours = {c.tobytes() for c in img[mask][:, :3]}
        assert {c.tobytes() for c in out[~mask][:, :3]} <= colours
        again, rec2 = R.bleed(out, 0.0, wrap)
        assert again.tobytes() == out.tobytes() and rec2 == rec


def test_no_seed_and_all_seeds_return_the_image():
    rng = np.random.default_rng(5)
    for mask in (np.zeros((9, 14), bool), np.ones((9, 14), bool)):
        for dtype in (np.uint8, np.float32):
            img = image_of(mask, dtype, 6)
            out, rec = R.bleed(img, 0.0, bool(rng.integers(2)))
            assert out.tobytes() == img.tobytes()
            assert rec == {"seeds": int(mask.sum()), "filled": 0, "max_dist2": 0, "reserved": 0}


def test_one_corner_seed():
    mask = np.zeros((8, 16), bool)
    mask[0, 0] = True
    img = image_of(mask, np.uint8, 7)
    out, rec = R.bleed(img)
    assert rec == {"seeds": 1, "filled": 127, "max_dist2": 15**2 + 7**2, "reserved": 0}
    assert (out[..., :3] == img[0, 0, :3]).all()
    out, rec = R.bleed(img, wrap=True)
    assert rec["filled"] == 127 and rec["max_dist2"] == 8**2 + 4**2
    assert R.bleed(img, wrap=(True, False))[1]["max_dist2"] == 8**2 + 7**2
    assert R.bleed(img, wrap=(False, True))[1]["max_dist2"] == 15**2 + 4**2


def test_a_tie_goes_to_the_smaller_seed_word():
    mask = np.zeros((5, 9), bool)
    mask[2, 1] = mask[2, 7] = True                  # (x, y) = (1, 2) and (7, 2): x = 4 is three texels from each
    img = image_of(mask, np.float32, 8)
    out, _ = R.bleed(img)
    assert out[2, 4, :3].tobytes() == img[2, 1, :3].tobytes()
    assert out[2, 5, :3].tobytes() == img[2, 7, :3].tobytes()
    mask = np.zeros((9, 5), bool)
    mask[1, 2] = mask[7, 2] = True                  # the word's high half is y: the upper seed is the smaller word
    img = image_of(mask, np.float32, 9)
    out, _ = R.bleed(img)
    assert out[4, 2, :3].tobytes() == img[1, 2, :3].tobytes()
    # (3, 0) and (0, 3) are equally far from (0, 0): the word 3 | 0 << 16 is the smaller
    mask = np.zeros((6, 6), bool)
    mask[0, 3] = mask[3, 0] = True
    img = image_of(mask, np.uint8, 10)
    img[0, 3, :3], img[3, 0, :3] = (1, 2, 3), (4, 5, 6)
    assert R.bleed(img)[0][0, 0, :3].tolist() == [1, 2, 3]


def test_max_distance_fills_exactly_the_near_texels():
    mask = np.zeros((17, 19), bool)
    mask[8, 9] = True
    img = image_of(mask, np.float16, 11)
    out, rec = R.bleed(img, max_distance=3)
    y, x = np.mgrid[0:17, 0:19]
    near = ((x - 9)**2 + (y - 8)**2 <= 9) & ~mask
    changed = (out.view(np.uint16) != img.view(np.uint16)).any(-1)
    assert rec["filled"] == near.sum() == 28 and rec["max_dist2"] == 9
    assert not changed[~near].any()
    assert (out[near][:, :3].view(np.uint16) == img[8, 9, :3].view(np.uint16)).all()


def test_nan_alpha_is_not_a_seed_and_bits_are_copied():
    img = np.zeros((4, 6, 4), np.float32)
    img[..., :3] = np.random.default_rng(12).random((4, 6, 3))
    img[1, 1, 3] = np.nan
    img[2, 4, 3] = 0.5
    img[2, 4, :3] = np.array([0x7FA00001, 0x80000000, 0x00000001], np.uint32).view(np.float32)   # a NaN payload, -0, a denormal
    out, rec = R.bleed(img)
    assert rec["seeds"] == 1 and rec["filled"] == 23
    assert (out[..., :3].view(np.uint32) == np.array([0x7FA00001, 0x80000000, 0x00000001], np.uint32)).all()
    assert out[..., 3].tobytes() == img[..., 3].tobytes()
    # negative and infinite alpha: -1 is no seed, +inf is
    img[1, 1, 3], img[0, 0, 3] = -1.0, np.inf
    assert R.bleed(img)[1]["seeds"] == 2


def test_threshold_on_rgba8():
    img = np.zeros((1, 4, 4), np.uint8)
    img[0, :, 3] = (127, 128, 0, 255)
    img[0, :, 0] = (10, 20, 30, 40)
    assert R.seed_mask(img, 0.5).tolist() == [[False, True, False, True]]
    out, rec = R.bleed(img, 0.5)
    assert rec["seeds"] == 2 and out[0, :, 0].tolist() == [20, 20, 20, 40]       # x = 2: a tie, the smaller word
    assert R.seed_mask(img, 0.0).tolist() == [[True, True, False, True]]
    with pytest.raises(ValueError):
        R.bleed(img, 1.0)
    with pytest.raises(ValueError):
        R.bleed(img, 0.0, max_distance=65536)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1)])
def test_degenerate_surfaces(h, w):
    for wrap in (False, True):
        mask = np.zeros((h, w), bool)
        img = image_of(mask, np.uint8, 13)
        assert R.bleed(img, wrap=wrap)[0].tobytes() == img.tobytes()
        mask[h//3, w//3] = True
        img = image_of(mask, np.uint8, 13)
        out, rec = R.bleed(img, wrap=wrap)
        assert rec["seeds"] == 1 and rec["filled"] == h*w - 1
        assert (out[..., :3] == img[h//3, w//3, :3]).all()
        far = max(h, w) - 1 - max(h, w)//3
        assert rec["max_dist2"] == (0 if h*w == 1 else (max(h, w)//2)**2 if wrap else far**2)
