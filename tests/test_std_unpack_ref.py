"""tests/std_unpack_ref.py, the numpy twin of the standard-format unpack, against hand-derived vectors (the words of
tests/test_oracle_stdpack.py read backwards) and against the unchanged forward packer oracle/std_pack.c through
round-trip laws over all 66 legal (format, type) pairs.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
import std_unpack_ref as R
from std_unpack_ref import F, FLOAT, INT, SNORM, UFLOAT, UINT, UNORM
from test_oracle_stdpack import ALL_PAIRS, LEGAL


def one(word, fmt, typ=UNORM, nbytes=None):
    """the texel of one pixel given as an integer word"""
    n = nbytes or R.pixel_bytes(fmt)
    return R.unpack(np.frombuffer(int(word).to_bytes(n, "little"), np.uint8), fmt, typ, 1, 1)[0, 0]


def f32(x):
    return np.float32(x)


def q(v, m):
    return f32(v)/f32(m)


def same(got, want):
    want = np.array(want, np.float32)
    assert got.dtype == np.float32
    assert np.array_equal(got, want), (got, want)


def test_all_66_pairs_have_a_pixel_size_that_matches_the_packer():
    assert len(ALL_PAIRS) == 66
    for f, t in ALL_PAIRS:
        assert R.pixel_bytes(f) == LEGAL[f][t] == O.std_pixel_bytes(f, t)


def test_known_answers_of_the_bit_field_formats():
    # the words of test_known_answers_of_the_bit_field_packers: r = 1, g = round(0.5*max), b = 0, a = 1
    same(one(8 | (15 << 4), F["R4G4"]), [1, q(8, 15), 0, 1])
    same(one(15 | (0 << 4) | (8 << 8) | (15 << 12), F["R4G4B4A4"]), [1, q(8, 15), 0, 1])
    same(one(15 | (15 << 4) | (8 << 8) | (0 << 12), F["B4G4R4A4"]), [1, q(8, 15), 0, 1])
    same(one(0 | (8 << 4) | (15 << 8) | (15 << 12), F["A4R4G4B4"]), [1, q(8, 15), 0, 1])
    same(one(0 | (32 << 5) | (31 << 11), F["R5G6B5"]), [1, q(32, 63), 0, 1])
    same(one(31 | (32 << 5) | (0 << 11), F["B5G6R5"]), [1, q(32, 63), 0, 1])
    same(one(1 | (0 << 1) | (16 << 6) | (31 << 11), F["R5G5B5A1"]), [1, q(16, 31), 0, 1])
    same(one(1 | (31 << 1) | (16 << 6) | (0 << 11), F["B5G5R5A1"]), [1, q(16, 31), 0, 1])
    same(one(0 | (16 << 5) | (31 << 10) | (1 << 15), F["A1R5G5B5"]), [1, q(16, 31), 0, 1])
    same(one(int.from_bytes(bytes([0, 128, 255]), "little"), F["B8G8R8"]), [1, q(128, 255), 0, 1])
    same(one(int.from_bytes(bytes([0, 128, 255, 255]), "little"), F["B8G8R8A8"]), [1, q(128, 255), 0, 1])
    same(one(int.from_bytes(bytes([255, 0, 128, 255]), "little"), F["A8B8G8R8"]), [1, q(128, 255), 0, 1])
    same(one(0 | (512 << 10) | (1023 << 20) | (3 << 30), F["A2R10G10B10"]), [1, q(512, 1023), 0, 1])
    same(one(1023 | (512 << 10) | (0 << 20) | (3 << 30), F["A2B10G10R10"]), [1, q(512, 1023), 0, 1])
    same(one(1023 | (8 << 10) | (1000 << 20) | (3 << 30), F["A2R10G10B10"], UINT), [1000, 8, 1023, 3])
    same(one(1000 | (8 << 10) | (1023 << 20) | (3 << 30), F["A2B10G10R10"], UINT), [1000, 8, 1023, 3])
    # alpha of one and two bits, off
    same(one(31 << 11, F["R5G5B5A1"]), [1, 0, 0, 0])
    same(one(1 << 30, F["A2B10G10R10"]), [0, 0, 0, q(1, 3)])


def words(vals, dtype):
    return int.from_bytes(np.array(vals, dtype).tobytes(), "little")


def test_known_answers_of_the_channel_arrays():
    same(one(words([0, 128, 255, 0], np.uint8), F["R8G8B8A8"]), [0, q(128, 255), 1, 0])
    same(one(words([-127, 64, 127, -32], np.int8), F["R8G8B8A8"], SNORM), [-1, q(64, 127), 1, q(-32, 127)])
    same(one(words([-128, -128, 1, 0], np.int8), F["R8G8B8A8"], SNORM), [-1, -1, q(1, 127), 0])
    same(one(words([0, 32768, 65535, 0], np.uint16), F["R16G16B16A16"]), [0, q(32768, 65535), 1, 0])
    same(one(words([-32767, 16384, 32767, -32768], np.int16), F["R16G16B16A16"], SNORM),
         [-1, q(16384, 32767), 1, -1])
    same(one(words([0, 3, 255, 255], np.uint8), F["R8G8B8A8"], UINT), [0, 3, 255, 255])
    same(one(words([-4, 3, 127, -128], np.int8), F["R8G8B8A8"], INT), [-4, 3, 127, -128])
    same(one(words([0, 3, 300, 65535], np.uint16), F["R16G16B16A16"], UINT), [0, 3, 300, 65535])
    same(one(words([-4, 3, 300, 32767], np.int16), F["R16G16B16A16"], INT), [-4, 3, 300, 32767])
    same(one(words([0, 3, 300, 70000], np.uint32), F["R32G32B32A32"], UINT), [0, 3, 300, 70000])
    same(one(words([-4, 3, 300, 70000], np.int32), F["R32G32B32A32"], INT), [-4, 3, 300, 70000])
    same(one(words([0xFFFFFFFF, 0x1000001, 0, 0], np.uint32), F["R32G32B32A32"], UINT), [4294967296.0, 16777216.0, 0, 0])
    v = np.array([-3.5, 2.5, 300.0, 70000.0], np.float32)
    same(one(words(v, np.float32), F["R32G32B32A32"], FLOAT), v)
    h = np.array([1.2, -3.4, 5.6, -7.8], np.float16)                       # HalfFloatTest.cpp's vector
    same(one(words(h, np.float16), F["R16G16B16A16"], FLOAT), h.astype(np.float32))
    # the narrower arrays: absent channels read 0, 0, 1
    same(one(200, F["R8"]), [q(200, 255), 0, 0, 1])
    same(one(words([200, 100], np.uint8), F["R8G8"]), [q(200, 255), q(100, 255), 0, 1])
    same(one(words([200, 100, 50], np.uint8), F["R8G8B8"]), [q(200, 255), q(100, 255), q(50, 255), 1])
    same(one(40000, F["R16"]), [q(40000, 65535), 0, 0, 1])
    same(one(words([-5, 7], np.int16), F["R16G16"], INT), [-5, 7, 0, 1])
    same(one(words([1.5, -2.0, 0.25], np.float16), F["R16G16B16"], FLOAT), [1.5, -2.0, 0.25, 1])
    same(one(words([-9], np.int32), F["R32"], INT), [-9, 0, 0, 1])
    same(one(words([1.25, -8.0], np.float32), F["R32G32"], FLOAT), [1.25, -8.0, 0, 1])
    same(one(words([7, 8, 9], np.uint32), F["R32G32B32"], UINT), [7, 8, 9, 1])
    # NaN stays NaN; a 32-bit float keeps its bits
    assert np.isnan(one(0x7E01, F["R16"], FLOAT)[0])
    got = one(0x7F800001, F["R32"], FLOAT)
    assert got.view(np.uint32)[0] == 0x7F800001


def test_known_answers_of_the_ufloat_formats():
    # test_b10g11r11_truncates...: px(0, inf, 1.0) packs to this word
    same(one(0 | ((31 << 6) << 11) | ((15 << 5) << 22), F["B10G11R11"], UFLOAT), [0, np.inf, 1, 1])
    same(one(0, F["B10G11R11"], UFLOAT), [0, 0, 0, 1])
    same(one((16 << 6) | 32, F["B10G11R11"], UFLOAT), [3.0, 0, 0, 1])                  # 1.5 * 2^1
    same(one(1 | (1 << 11) | (1 << 22), F["B10G11R11"], UFLOAT), [2.0**-20, 2.0**-20, 2.0**-19, 1])   # denormals
    same(one(63 | (31 << 22), F["B10G11R11"], UFLOAT), [63*2.0**-20, 0, 31*2.0**-19, 1])
    same(one(((30 << 6) | 63) | (((30 << 5) | 31) << 22), F["B10G11R11"], UFLOAT), [65024.0, 0, 64512.0, 1])  # largest
    got = one(((31 << 6) | 1) | (((31 << 5) | 7) << 22), F["B10G11R11"], UFLOAT)
    assert np.isnan(got[0]) and got[1] == 0 and np.isnan(got[2]) and got[3] == 1
    same(one((31 << 5) << 22, F["B10G11R11"], UFLOAT), [0, 0, np.inf, 1])
    # E5B9G9R9: m * 2^(e - 24)
    same(one(0, F["E5B9G9R9"], UFLOAT), [0, 0, 0, 1])
    same(one(256 | (16 << 27), F["E5B9G9R9"], UFLOAT), [1, 0, 0, 1])
    same(one((256 << 18) | (16 << 27), F["E5B9G9R9"], UFLOAT), [0, 0, 1, 1])
    same(one(256 | (31 << 27), F["E5B9G9R9"], UFLOAT), [32768.0, 0, 0, 1])
    same(one(1 | (2 << 9) | (511 << 18), F["E5B9G9R9"], UFLOAT), [2.0**-24, 2.0**-23, 511*2.0**-24, 1])   # exponent 0
    same(one(511 | (31 << 27), F["E5B9G9R9"], UFLOAT), [65408.0, 0, 0, 1])               # above the packer's clamp


# ---- round-trip laws against the forward packer -------------------------------------------------------

def patterns(fmt, typ):
    """(payload bytes, w, h): every word for pixels of at most 16 bits, 2^20 seeded random words otherwise"""
    bpp = R.pixel_bytes(fmt)
    if bpp <= 2:
        n = 1 << (8*bpp)
        p = np.arange(n, dtype=np.uint32).astype("<u%d" % bpp).view(np.uint8)
        return p, (16, 16) if bpp == 1 else (256, 256)
    rng = np.random.default_rng(1000*fmt + typ)
    p = rng.integers(0, 256, size=(1 << 20)*bpp, dtype=np.uint8)
    if bpp % 4 == 0 and R.fields(fmt)[0][2] == 32 and typ in (UINT, INT):
        # half of the 32-bit integers below 2^24 in magnitude, where float holds them exactly
        w = p.view("<u4").copy()
        small = rng.random(w.size) < 0.5
        if typ == INT:
            w[small] = (w[small].view(np.int32) >> 8).view(np.uint32)
        else:
            w[small] >>= 8
        p = w.view(np.uint8)
    return p, (1024, 1024)


def field_of(payload, fmt, shift, bits):
    lo, hi = R.pixel_words(payload, fmt, 0)
    src, s = (lo, shift) if shift < 64 else (hi, shift - 64)
    return (src >> np.uint64(s)) & np.uint64(2**bits - 1)


@pytest.mark.parametrize("fmt,typ", ALL_PAIRS)
def test_round_trip_laws(fmt, typ):
    p, (w, h) = patterns(fmt, typ)
    tex = R.unpack(p, fmt, typ, w, h)
    assert tex.dtype == np.float32 and tex.shape == (h, w, 4)
    name = R.NAME[fmt]
    stored = {c for c, _, _ in R.fields(fmt)}
    for c in range(4):                                   # absent channels: 0, 0, 1
        if c not in stored:
            assert np.all(tex[..., c] == (1.0 if c == 3 else 0.0))
    if name == "E5B9G9R9":
        # not canonical: the law is on values, for words the packer's clamp (32768) does not change
        back = R.unpack(O.std_pack(tex, fmt, typ), fmt, typ, w, h)
        keep = tex[..., :3].max(axis=2) <= 32768.0
        assert 1.0 - keep.mean() <= 1.0/32.0
        assert np.array_equal(back[keep], tex[keep])
        return
    if typ == FLOAT and R.fields(fmt)[0][2] == 32:
        assert np.array_equal(tex.view(np.uint32)[..., :len(stored)].ravel(), p.view("<u4"))   # bits, NaN included
        assert np.array_equal(O.std_pack(tex, fmt, typ), p)
        return
    with np.errstate(invalid="ignore"):
        again = O.std_pack(tex, fmt, typ)
    for c, shift, bits in R.fields(fmt):
        v = field_of(p, fmt, shift, bits)
        v2 = field_of(again, fmt, shift, bits)
        val = tex[..., c].ravel()
        keep = np.ones(v.shape, bool)
        if name == "B10G11R11":
            mb = bits - 5
            e, m = v >> np.uint64(mb), v & np.uint64(2**mb - 1)
            keep = ~(((e == 0) | (e == 31)) & (m != 0))                   # denormal and NaN fields
            ae = np.arange(2**bits) >> mb
            am = np.arange(2**bits) & (2**mb - 1)
            assert int((((ae == 0) | (ae == 31)) & (am != 0)).sum()) == {10: 62, 11: 126}[bits]
        elif typ == SNORM:
            worst = np.uint64(1 << (bits - 1))                            # the one excluded pattern per field
            keep = v != worst
            assert np.all(val[~keep] == -1.0)
            assert np.all(v2[~keep] == worst + np.uint64(1))              # -127 / -32767
        elif typ == FLOAT:                                                # 16-bit halves
            nan = ((v >> np.uint64(10)) & np.uint64(31) == 31) & (v & np.uint64(1023) != 0)
            keep = ~nan
            assert np.all(np.isnan(val[nan])) and not np.any(np.isnan(val[keep]))
            if (w, h) == (256, 256) and name == "R16":
                assert int(keep.sum()) == 63490
        elif bits == 32:                                                  # UInt / Int
            signed = v.astype(np.int64) - ((v >> np.uint64(31)).astype(np.int64) << 32) if typ == INT \
                else v.astype(np.int64)
            keep = np.abs(signed) <= (1 << 24)
            assert keep.mean() > 0.4
            assert np.array_equal(val, signed.astype(np.float32))         # everywhere: float32(p), nearest even
        assert np.array_equal(v2[keep], v[keep]), (name, typ, c)


# ---- the kernel's division-free quotient ---------------------------------------------------------------

@pytest.mark.parametrize("maxv", [1, 3, 15, 31, 63, 127, 255, 1023, 32767, 65535])
def test_the_kernels_newton_quotient_is_the_rounded_quotient(maxv):
    # std_unpack.h: q = x*(1/MAX); q += fma(-q, MAX, x)*(1/MAX) -- must equal float32(x)/float32(MAX) for every
    # x the kernel feeds it: 0..MAX for UNorm, -(MAX+1)..MAX for SNorm (127, 32767)
    lo = -(maxv + 1) if maxv in (127, 32767) else 0
    x = np.arange(lo, maxv + 1, dtype=np.float64)
    r = np.float64(np.float32(1.0)/np.float32(maxv))
    q0 = (x*r).astype(np.float32).astype(np.float64)              # 24 x 24 bit product: exact in double, one rounding
    rem = (x - q0*maxv).astype(np.float32).astype(np.float64)     # fma: exact in double, one rounding
    t = rem*r                                                     # exact in double
    q1 = (t + q0).astype(np.float32)
    want = x.astype(np.float32)/np.float32(maxv)
    # the double sum t + q0 is itself rounded: it may only change the float result if it lands on a float tie
    assert np.array_equal(q1, want)
    assert np.array_equal((np.nextafter(t + q0, np.inf)).astype(np.float32), want)
    assert np.array_equal((np.nextafter(t + q0, -np.inf)).astype(np.float32), want)
