"""The numpy twin of the signed distance field (tests/alpha_sdf_ref.py) against the definition's own words: its windowed
two-pass e equals the brute-force minimum over all pairs exactly, its laws hold, and the field does what it is for --
a 32^2 field magnifies to a far better 256^2 edge than a 32^2 box-filtered alpha."""
import numpy as np
import pytest

import alpha_sdf_ref as R

WRAPS = [(False, False), (True, False), (False, True), (True, True)]
SIZES = [(7, 13), (16, 16), (5, 70), (40, 33)]            # (h, w)


def mask_of(h, w, density, seed):
    if density is True or density is False:
        return np.full((h, w), density)
    return np.random.default_rng(seed).random((h, w)) < density


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("spread", [1, 4, 16, 126])
def test_window_equals_brute_force(h, w, spread):
    k2 = (spread + 1)**2
    for i, density in enumerate((0.02, 0.5, 0.97, True, False)):
        mask = mask_of(h, w, density, 100*h + w + i)
        for wrap in WRAPS:
            e = R.squared_distance(mask, spread, wrap)
            assert e.dtype == np.int64 and (e == R.brute_force(mask, spread, wrap)).all(), (density, wrap)
            assert e.min() >= 1 and e.max() <= k2
            if density is True or density is False:
                assert (e == k2).all()


def test_swapping_the_classes_mirrors_the_field():
    for (h, w), scale in (((16, 16), 1), ((40, 32), 4), ((32, 64), 16)):
        mask = mask_of(h, w, 0.4, h)
        for wrap in WRAPS:
            # the distances and the tile means mirror exactly; v = 0.5 + m / (2 spread) to the one rounding of its sum,
            # and exactly where the division is exact (a spread that is a power of two)
            for spread in (5, 4):
                v, e = R.field_of_mask(mask, spread, scale, wrap)
                v2, e2 = R.field_of_mask(~mask, spread, scale, wrap)
                m, m2 = (R.tile_mean(R.signed_distance(e, c), scale) for c in (mask, ~mask))
                assert (e == e2).all() and (m2 == -m).all() and 0.0 < v.min() and v.max() < 1.0
                assert np.abs(v2 - (1.0 - v)).max() <= (2.0**-53 if spread == 5 else 0.0)


@pytest.mark.parametrize("wrap", WRAPS)
def test_a_single_inside_texel(wrap):
    h, w, spread = 9, 21, 6
    k2 = (spread + 1)**2
    for px, py in ((0, 0), (20, 8), (10, 4), (1, 7)):
        mask = np.zeros((h, w), bool)
        mask[py, px] = True
        y, x = np.mgrid[0:h, 0:w]
        dx, dy = np.abs(x - px), np.abs(y - py)
        if wrap[0]:
            dx = np.minimum(dx, w - dx)
        if wrap[1]:
            dy = np.minimum(dy, h - dy)
        want = np.minimum(k2, dx*dx + dy*dy)
        want[py, px] = 1                                   # the texel itself: its nearest outside neighbour
        assert (R.squared_distance(mask, spread, wrap) == want).all()


def test_saturated_tiles_reach_exactly_0_and_1():
    mask = np.zeros((64, 96), bool)
    mask[:, 48:] = True
    for spread, scale in ((3, 4), (7, 8), (1, 2), (15, 16)):
        v, e = R.field_of_mask(mask, spread, scale)
        sat = (e == (spread + 1)**2).reshape(64//scale, scale, 96//scale, scale).all((1, 3))
        assert sat.any() and set(np.unique(v[sat]).tolist()) == {0.0, 1.0}
        assert ((v[sat] == 1.0) == mask[::scale, ::scale][sat]).all()
        for dtype in (np.uint8, np.float16, np.float32):
            q = R.quantise(v, dtype)
            assert set(np.unique(q[sat]).tolist()) == {0, 255 if dtype == np.uint8 else 1}


def test_the_tile_sum_does_not_depend_on_the_order():
    mask = mask_of(64, 64, 0.5, 3)
    e = R.squared_distance(mask, 126)
    e[::3, ::5] = 127*127                                  # the largest values among the smallest
    sd = R.signed_distance(e, mask)
    assert (sd*2.0**23 == np.round(sd*2.0**23)).all() and np.abs(sd).max() < 128.0
    tiles = sd.reshape(4, 16, 4, 16).transpose(0, 2, 1, 3).reshape(4, 4, 256)
    rng = np.random.default_rng(4)
    sums = []
    for order in (np.arange(256), np.arange(256)[::-1], rng.permutation(256)):
        acc = np.zeros((4, 4))
        for i in order:
            acc = acc + tiles[..., i]
        sums.append(acc)
    assert sums[0].tobytes() == sums[1].tobytes() == sums[2].tobytes() == tiles.sum(-1).tobytes()
    assert (R.tile_mean(sd, 16)*256.0).tobytes() == sums[0].tobytes()


def test_quantisation_and_channels():
    v = np.array([[0.0, 0.5, 1.0, 127.5/255, 0.1]])
    assert R.quantise(v, np.uint8).tolist() == [[0, 128, 255, 128, 26]]
    assert R.quantise(v, np.float16).dtype == np.float16 and R.quantise(v, np.float32)[0, 4] == np.float32(0.1)
    assert [R.channel_mask(c) for c in ("a", "r", "rgba", "gb", 5)] == [8, 1, 15, 6, 5]
    dst = np.arange(20, dtype=np.uint8).reshape(1, 5, 4)
    out = R.apply(dst, R.quantise(v, np.uint8), "gb")
    assert (out[..., (0, 3)] == dst[..., (0, 3)]).all() and out[0, :, 1].tolist() == out[0, :, 2].tolist() == [0, 128, 255, 128, 26]
    img = np.zeros((2, 2, 4), np.float32)
    img[0, 0, 3] = np.nan
    img[1, 1, 3] = 0.5000001
    img[0, 1, 3] = 0.5
    assert R.inside_mask(img, 0.5).tolist() == [[False, False], [False, True]]
    with pytest.raises(ValueError):
        R.field_of_mask(np.zeros((6, 8), bool), 3, 4)
    with pytest.raises(ValueError):
        R.field_of_mask(np.zeros((8, 8), bool), 127)


def test_the_field_magnifies_better_than_box_filtered_alpha():
    """three 256^2 masks to 32^2 at scale 8 and spread 8 as RGBA8, magnified bilinearly by 8 and cut at 0.5: at most half
    the wrong texels of the box-filtered alpha on the disc and the bar, fewer on the star (its tips are thinner than an
    output texel).  These masks: 43 / 189, 60 / 188, 294 / 431"""
    got = {}
    for name, mask in R.shapes().items():
        img = np.zeros(mask.shape + (4,), np.uint8)
        img[..., 3] = mask*255
        field, rec = R.sdf(img, 8, 8)
        assert field.dtype == np.uint8 and field.shape == (32, 32) and rec["inside"] == mask.sum()
        got[name] = (R.mismatches(field/255.0, mask), R.mismatches(R.box_alpha(mask, 8), mask))
        print("%s: field %d, box-filtered alpha %d wrong texels" % ((name,) + got[name]))
    assert 2*got["disc"][0] <= got["disc"][1] and 2*got["bar"][0] <= got["bar"][1]
    assert got["star"][0] < got["star"][1]
