"""The ETC1 / ETC2 / EAC cases of tests/etc_cases.py on the CPU oracle alone: the sources reach what they claim to
reach, and the oracle keeps the laws the HIP kernels are then held to (tests/test_gpu_etc_modes.py)."""
import numpy as np
import pytest

import etc_cases as C
import oracle_lib as O
from cuttlefish_amd import synth

COLOUR = [C.ETC1, C.RGB, C.A1, C.A8]
EAC = [(C.R11, C.UNORM), (C.R11, C.SNORM), (C.RG11, C.UNORM), (C.RG11, C.SNORM)]


def _enc(img, fmt, typ=0, quality=2, **kw):
    return O.encode(img, int(fmt), typ=int(typ), quality=quality, threads=8, **kw)


def test_classifiers_on_hand_built_blocks():
    indiv = np.array([0xF0, 0xF0, 0xF0, 0x01, 0, 0, 0, 0], np.uint8)            # differential bit clear, flip set
    assert [int(v[0]) for v in C.mode_of(indiv)] == [C.INDIVIDUAL, 1]
    assert [int(v[0]) for v in C.mode_of(indiv, a1=True)] == [C.DIFFERENTIAL, 1]   # RGB8A1: a punch-through block
    assert C.opaque_flag(indiv)[0] == 0
    t = np.array([0x04, 0, 0, 0x02, 0, 0, 0, 0], np.uint8)                       # R = 0, dR = -4
    h = np.array([0, 0x04, 0, 0x02, 0, 0, 0, 0], np.uint8)                       # G = 0, dG = -4
    p = np.array([0, 0, 0x04, 0x02, 0, 0, 0, 0], np.uint8)                       # B = 0, dB = -4
    d = np.array([0x08, 0x08, 0x08, 0x02, 0, 0, 0, 0], np.uint8)
    assert list(C.mode_of(np.stack([t, h, p, d]))[0]) == [C.T, C.H, C.PLANAR, C.DIFFERENTIAL]
    assert list(C.class_of(np.stack([indiv, t, h, p, d]))) == [1, 4, 5, 6, 2]
    assert [C.etc_mode(b) for b in (indiv, t, h, p, d)] == [0, 1, 2, 3, 0]
    base, mult, table = C.eac_fields(np.array([0x81, 0x2D, 0, 0, 0, 0, 0, 0], np.uint8), signed=True)
    assert (base[0], mult[0], table[0]) == (-127, 2, 13)
    assert C.eac_fields(np.array([0x81, 0x2D, 0, 0, 0, 0, 0, 0], np.uint8))[0][0] == 0x81


def test_sources_are_what_they_say():
    src = C.colour_source()
    assert src.shape == (64, 112, 4) and src.dtype == np.uint8 and (src[..., 3] == 255).all()
    assert C.colour_source(wide=True).shape == (48, 144, 4)
    a1 = C.a1_source()
    assert (a1[:16, :, 3] == 255).all() and set(np.unique(a1[..., 3])) == {0, 255}
    assert 0.2 < (a1[16:, :, 3] == 0).mean() < 0.3
    for typ in (C.UNORM, C.SNORM):
        f = C.eac_source(typ)
        assert f.shape == (64, 112, 4) and f.dtype == np.float32
        lv = C.r11_levels(f, typ, 2)
        assert np.array_equal(lv[..., 1], lv[:, ::-1, 0])
        assert lv.min() == (-1023 if typ else 0) and lv.max() == (1023 if typ else 2047)
    a8 = C.a8_source()
    assert np.array_equal(a8[..., :3], src[..., :3]) and a8[..., 3].min() == 0 and a8[..., 3].max() == 255


@pytest.mark.parametrize("quality", C.LEVELS)
@pytest.mark.parametrize("fmt", COLOUR)
def test_mode_counts(fmt, quality):
    src = {C.A1: C.a1_source, C.A8: C.a8_source}.get(fmt, C.colour_source)()
    payload = _enc(src, fmt, 0, quality)
    C.check_mode_counts(payload, fmt, quality)
    dec = O.decode_etc(payload, fmt, src.shape[1], src.shape[0])
    if fmt == C.A1:                                                              # the alpha mask survives exactly
        assert np.array_equal(dec[..., 3], src[..., 3])
    elif fmt == C.A8:
        base, mult, table = C.eac_fields(payload.reshape(-1, 16)[:, :8])
        assert (np.bincount(table, minlength=16) >= 8).all() and (np.bincount(mult, minlength=16)[1:] >= 4).all()
        assert (base <= 8).any() and (base >= 249).any()


@pytest.mark.parametrize("quality", C.LEVELS)
@pytest.mark.parametrize("fmt,typ", EAC)
def test_eac_counts(fmt, typ, quality):
    C.check_eac_counts(_enc(C.eac_source(typ), fmt, typ, quality), typ)


@pytest.mark.parametrize("quality", C.LEVELS)
def test_flat_laws(quality):
    C.check_flat_alpha_law(_enc, quality)
    for fmt in COLOUR:
        C.check_flat_colour_law(_enc, fmt, quality)
    for fmt, typ in EAC:
        C.check_flat_r11_law(_enc, fmt, typ, quality)


def test_the_etc1_flat_maxima_are_the_oracles_own():
    img = C.flat_colours()
    for q in C.LEVELS:
        dec = O.decode_etc(_enc(img, C.ETC1, 0, q), C.ETC1, img.shape[1], img.shape[0])
        assert np.abs(dec[..., :3].astype(int) - img[..., :3]).max() == C.ETC1_FLAT_MAX[q]


@pytest.mark.parametrize("typ", [C.UNORM, C.SNORM])
def test_no_eac_block_is_worse_than_the_flat_block(typ):
    photo = C.as_float(synth.photo(128, 64, seed=5))
    sources = [C.eac_source(typ), photo*2 - 1 if typ else photo, C.as_float(C.noise_image())]
    for i, src in enumerate(sources):
        vals = C.r11_levels(src, typ, 2)
        for q in C.LEVELS:
            assert C.over_flat_bound_eac(_enc(src, C.RG11, typ, q), vals, typ, C.RG11) == (0, 0.0), (i, q)
    a8 = C.a8_source()
    for q in C.LEVELS:
        assert C.over_flat_bound_eac(_enc(a8, C.A8, 0, q), a8[..., 3], 0, C.A8) == (0, 0.0), q


@pytest.mark.parametrize("fmt", COLOUR)
def test_no_colour_block_is_worse_than_the_flat_block(fmt):
    bad = []
    for name, img in C.bound_sources():
        for q in range(C.BOUND_FROM[fmt], 5):
            n, ratio = C.over_flat_bound_rgb(_enc(img, fmt, 0, q), img, fmt)
            if n:
                bad.append("%s level %d: %d blocks, worst %.2f x the flat block" % (name, q, n, ratio))
    assert not bad, "\n".join(bad)


def test_the_flat_bound_is_the_error_of_a_block_the_format_holds():
    """the bound's own arithmetic against the decoder: the flat candidate written out as a differential block"""
    img = np.ascontiguousarray(synth.photo(16, 4, seed=2, alpha=False))
    bound = C.flat_bound_rgb(img)
    px = C._blocks(img[..., :3].astype(np.int64))
    for i in range(4):
        q = ((2*px[i].sum(axis=0) + 16)//32*31 + 127)//255
        best = None
        for t in range(8):
            hi = (int(q[0]) << 27) | (int(q[1]) << 19) | (int(q[2]) << 11) | (t << 5) | (t << 2) | 2
            base = (q << 3) | (q >> 2)
            lo = 0
            for x in range(4):
                for y in range(4):
                    mods = [C.ETC_MOD[t][0], C.ETC_MOD[t][1], -C.ETC_MOD[t][0], -C.ETC_MOD[t][1]]
                    e = [((np.clip(base + m, 0, 255) - px[i][4*y + x])**2).sum() for m in mods]
                    s = int(np.argmin(e))
                    lo |= ((s >> 1) << (16 + 4*x + y)) | ((s & 1) << (4*x + y))
            blk = np.frombuffer(hi.to_bytes(4, "big") + lo.to_bytes(4, "big"), np.uint8)
            assert C.mode_of(blk)[0][0] == C.DIFFERENTIAL
            d = O.decode_etc(blk, C.RGB, 4, 4)[..., :3].astype(np.int64) - img[:, 4*i:4*i + 4, :3]
            best = int((d*d).sum()) if best is None else min(best, int((d*d).sum()))
        assert best == bound[i]


@pytest.mark.parametrize("fmt", COLOUR)
def test_unorm8_boundaries(fmt):
    C.check_unorm8_law(_enc, fmt, 1)


@pytest.mark.parametrize("fmt,typ", EAC)
def test_r11_boundaries(fmt, typ):
    C.check_r11_law(_enc, fmt, typ, 1)


def test_the_loaders_in_numpy():
    f = C.unorm8_boundaries()
    assert f.dtype == np.float32 and f.size == 255*3 + 11 and np.isnan(f).sum() == 2
    assert np.signbit(f[np.isnan(f)]).tolist() == [False, True]
    lv = C.unorm8_levels(f)
    assert lv[:6].tolist() == [0, 1, 1, 1, 2, 2] and lv[-11:].tolist() == [0, 255, 0, 0, 255, 0, 0, 255, 0, 0, 0]
    for snorm in (False, True):
        g = C.r11_boundaries(snorm)
        lv = C.r11_levels(g.reshape(1, -1, 1), int(snorm), 1).reshape(-1)
        top = 1023 if snorm else 2047
        assert lv[-11:].tolist() == [0, top, -top if snorm else 0, 0, top, -top if snorm else 0, 0, top,
                                     -top if snorm else 0, 0, 0]
        # every tie rounds away from zero unless float32 puts the product on the other side of the half
        assert set(np.unique(lv)) == set(range(-top if snorm else 0, top + 1))


@pytest.mark.parametrize("typ", [C.UNORM, C.SNORM])
def test_a_nan_texel_is_level_zero(typ):
    """one NaN in a block of 0.5: the NaN texel is level 0, like the colour loader's, the others round(0.5 * 2047) =
    1024 (signed: 512)"""
    f = np.full((4, 4, 4), 0.5, np.float32)
    f[1, 2, 0] = np.nan
    for q in C.LEVELS:
        p = _enc(f, C.R11, typ, q)
        g = f.copy()
        g[1, 2, 0] = 0
        assert np.array_equal(p, _enc(g, C.R11, typ, q))
        want = C.r11_levels(f, typ, 1)[..., 0]
        assert want[1, 2] == 0 and want[0, 0] == (512 if typ else 1024)
        # the block is no worse than the flat block of these levels: the 15 texels are not given up for the one
        assert C.over_flat_bound_eac(p, want[..., None], typ) == (0, 0.0)


def test_special_values_in_a_photo_are_the_loaders():
    f = C.sprinkle_specials(synth.photo(68, 44, seed=12))
    assert np.isnan(f).any() and np.isinf(f).any() and f.dtype == np.float32
    u8 = C.unorm8_levels(f)
    for fmt in COLOUR:
        assert np.array_equal(_enc(f, fmt, 0, 2), _enc(u8, fmt, 0, 2))
