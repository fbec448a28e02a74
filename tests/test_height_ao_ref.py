"""tests/height_ao_ref.py, the numpy twin of cfhip_height_ao_array_device, without a GPU: against a plain triple loop
bit for bit, and against what the definition must give -- a flat surface, a V-groove's closed form, a quarter turn, the
reach R_d, negative heights, strength and bias."""
import math

import numpy as np
import pytest

import height_ao_ref as ref


def loop_occlusion(h, radius, height, D, strength, bias, flags):
    """the definition, texel by texel, direction by direction, sample by sample"""
    rows, cols = h.shape
    vx, vy, wd = ref.directions(D)
    hs, b, s = np.float64(np.float32(height)), np.float64(np.float32(bias)), np.float64(np.float32(strength))
    v = np.zeros((rows, cols), np.float64)
    occ = np.zeros((rows, cols), bool)
    for y in range(rows):
        for x in range(cols):
            Hp = hs*np.float64(h[y, x])
            S = np.float64(0.0)
            for d in range(D):
                n = int(vx[d])**2 + int(vy[d])**2
                m = None
                k = 1
                while k*k*n <= radius*radius:
                    qx, qy = x + k*int(vx[d]), y + k*int(vy[d])
                    inside = True
                    if flags & ref.WRAP_X:
                        qx %= cols
                    elif not 0 <= qx < cols:
                        inside = False
                    if flags & ref.WRAP_Y:
                        qy %= rows
                    elif not 0 <= qy < rows:
                        inside = False
                    if inside:
                        g = np.float64(1.0)/(np.float64(k)*np.sqrt(np.float64(n)))
                        if flags & ref.FALLOFF:
                            g = g*(np.float64(1.0) - np.float64(k*k*n)/np.float64((radius + 1)**2))
                        c = (hs*np.float64(h[qy, qx]) - Hp)*g
                        m = c if m is None or c > m else m
                    k += 1
                t = np.float64(0.0) if m is None else max(np.float64(0.0), m - b)
                occ[y, x] |= t > 0.0
                if flags & ref.UNIFORM:
                    vis = np.float64(1.0) - t/np.sqrt(np.float64(1.0) + t*t)
                else:
                    vis = np.float64(1.0)/(np.float64(1.0) + t*t)
                S = S + wd[d]*vis
            v[y, x] = min(np.float64(1.0), max(np.float64(0.0), np.float64(1.0) - s*(np.float64(1.0) - S)))
    return v, occ


@pytest.mark.parametrize("D", (8, 16, 32))
def test_twin_equals_the_triple_loop(D):
    rng = np.random.default_rng(1000 + D)
    for flags in range(16):                                # both wraps, both visibilities, falloff on and off
        h = rng.standard_normal((7, 9)).astype(np.float32)*3.0
        radius = int(rng.integers(1, 12))
        kw = dict(radius=radius, height=float(rng.uniform(-2, 2)), D=D, strength=float(rng.uniform(0, 2)),
                  bias=float(rng.uniform(0, 0.3)), flags=flags)
        v, occ = ref.occlusion(h, **kw)
        lv, locc = loop_occlusion(h, **kw)
        assert v.tobytes() == lv.tobytes(), (D, flags, radius)
        assert (occ == locc).all()


def test_direction_tables():
    sectors = {8: (45, 45), 16: (26.565, 22.5, 18.435, 22.5),
               32: (18.435, 13.283, 7.628, 9.217, 11.310, 9.217, 7.628, 13.283)}
    for D, deg in sectors.items():
        vx, vy, w = ref.directions(D)
        assert len(vx) == len(vy) == len(w) == D
        assert [(int(x), int(y)) for x, y in zip(vx[:D//4], vy[:D//4])] == list(ref.BASES[D])
        for d in range(D):                                 # a quarter turn on: (x, y) -> (-y, x)
            assert (vx[(d + D//4) % D], vy[(d + D//4) % D]) == (-vy[d], vx[d])
            assert w[(d + D//4) % D] == w[d]
        ang = np.arctan2(vy, vx) % (2*math.pi)
        assert (np.diff(ang) > 0).all()                    # counter-clockwise from +x
        assert np.allclose(w[:D//4]*360.0, deg, atol=5e-4)
        assert abs(float(np.sum(w)) - 1.0) <= 2.0**-50 and ref.in_order_sum(w) == 1.0


def test_flat_surface_is_exactly_one():
    for D in (8, 16, 32):
        for flags in (0, ref.UNIFORM, ref.WRAP_X | ref.WRAP_Y | ref.FALLOFF):
            v, occ = ref.occlusion(np.full((11, 13), 0.75, np.float32), 9, 3.0, D, 2.0, 0.0, flags)
            assert (v == 1.0).all() and not occ.any()
    out, rec = ref.height_ao(np.full((5, 6, 4), 77, np.uint8), np.zeros((5, 6, 4), np.float32), 4, mask=5)
    assert (out[..., 0] == 1.0).all() and (out[..., 2] == 1.0).all() and not out[..., 1].any() and not out[..., 3].any()
    assert rec == dict(occluded=0, darkest=0x3F800000, reserved0=0, reserved1=0)


# measured with this definition; the closed form of a groove of slope s seen from its bottom, cosine-weighted
GROOVE = {0.5: (0.894427, (0.894444, 0.894153, 0.894260)),
          1.0: (0.707107, (0.708333, 0.705153, 0.705791)),
          2.0: (0.447214, (0.466667, 0.443791, 0.442633))}


@pytest.mark.parametrize("s", sorted(GROOVE))
def test_v_groove_bottom(s):
    closed, pinned = GROOVE[s]
    assert abs(closed - 1.0/math.sqrt(1.0 + s*s)) < 1e-6
    h = np.tile((s*np.abs(np.arange(65) - 32)).astype(np.float32), (65, 1))
    for D, pin in zip((8, 16, 32), pinned):
        v = ref.occlusion(h, 32, 1.0, D)[0][32, 32]
        assert abs(v - pin) <= 1e-6, (s, D, v)
        assert abs(v - closed) <= (0.02 if D == 8 else 0.005), (s, D, v)


def test_quarter_turn_turns_the_result():
    rng = np.random.default_rng(7)
    h = rng.standard_normal((12, 17)).astype(np.float32)
    for D in (8, 16, 32):
        for flags in (0, ref.WRAP_X, ref.UNIFORM | ref.FALLOFF):
            # np.rot90 moves the x axis onto the y axis, so a wrap flag moves with it
            turned = (flags & ~3) | (ref.WRAP_Y if flags & ref.WRAP_X else 0) | (ref.WRAP_X if flags & ref.WRAP_Y else 0)
            v = ref.occlusion(h, 6, 1.5, D, 1.0, 0.05, flags)[0]
            t = ref.occlusion(np.rot90(h).copy(), 6, 1.5, D, 1.0, 0.05, turned)[0]
            assert np.abs(np.rot90(v) - t).max() <= 1e-13


def test_reach_is_decided_in_integers():
    assert [ref.reach(2, 1, 0), ref.reach(2, 1, 1), ref.reach(2, 2, 1), ref.reach(3, 2, 1), ref.reach(64, 3, 2)] == \
        [2, 1, 0, 1, 17]
    assert ref.reach(5, 3, 4) == 1 and ref.reach(5, 4, 3) == 1 and ref.reach(1, 1, 1) == 0
    # at R = 2 the (2, 1) family has no sample: a wall everywhere but under the axes and diagonals changes nothing
    h = np.zeros((9, 9), np.float32)
    for x, y in ((2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)):
        h[4 + y, 4 + x] = 100.0
    v16 = ref.occlusion(h, 2, 1.0, 16)[0]
    assert v16[4, 4] == 1.0
    vx, vy, w = ref.directions(16)
    spike = np.zeros((9, 9), np.float32)
    spike[4, 5:] = 1e6                                      # direction 0 blocked, to the precision of a double
    got = ref.occlusion(spike, 2, 1.0, 16)[0][4, 4]
    assert abs(got - (1.0 - w[0])) < 1e-11
    assert ref.occlusion(h, 3, 1.0, 16)[0][4, 4] < 0.6      # one texel more and the family counts


def test_negative_height_is_negated_heights():
    rng = np.random.default_rng(11)
    h = rng.standard_normal((8, 10)).astype(np.float32)
    for D in (8, 32):
        a = ref.occlusion(h, 5, -1.25, D, 1.0, 0.01, ref.WRAP_X)[0]
        b = ref.occlusion(-h, 5, 1.25, D, 1.0, 0.01, ref.WRAP_X)[0]
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() != ref.occlusion(h, 5, 1.25, D, 1.0, 0.01, ref.WRAP_X)[0].tobytes()


def test_strength_zero_and_a_bias_above_every_slope():
    rng = np.random.default_rng(12)
    h = rng.uniform(0, 1, (8, 10)).astype(np.float32)
    v, occ = ref.occlusion(h, 5, 4.0, 16, 0.0)
    assert (v == 1.0).all() and occ.any()                   # the horizons are there, the strength hides them
    v, occ = ref.occlusion(h, 5, 4.0, 16, 1.0, 4.5)         # no slope exceeds height * range / 1 texel = 4
    assert (v == 1.0).all() and not occ.any()
    v = ref.occlusion(h, 5, 4.0, 16, 2.5)[0]
    assert v.min() == 0.0 and v.max() <= 1.0                # clamped at 0


def test_decode_and_store():
    img = np.zeros((1, 4, 4), np.float32)
    img[0, :, 2] = (np.nan, np.inf, -np.inf, 1e-40)
    h = ref.decode(img, 2)
    assert h.dtype == np.float32 and h[0, :3].tolist() == [0.0, 0.0, 0.0] and h[0, 3] == np.float32(1e-40)
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 64, 4)
    assert ref.decode(u8, 1)[0, 10] == np.float32(41/255.0)
    assert ref.decode(np.full((1, 1, 4), 0.5, np.float16), 3).dtype == np.float32
    v = np.array([0.0, 0.5, 0.49803921568627446, 1.0, 0.25098])
    assert ref.stored(v, np.uint8).tolist() == [0, 128, 127, 255, 64]
    assert ref.stored(v, np.float16).dtype == np.float16 and ref.stored(v, np.float32)[1] == np.float32(0.5)
