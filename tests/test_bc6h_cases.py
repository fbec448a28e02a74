"""BC6H on the CPU oracle alone: the conditions tests/test_gpu_bc6h_modes.py relies on (every mode is reached),
and the laws that tie what the encoder writes to what the decoder reads -- flat blocks are exact, the 8-bit and
float32 loaders round like numpy, and no block is worse than the constant block at its mean."""
import numpy as np
import pytest

import bc6h_cases as C
import oracle_lib as O

BC6H = 35
TYPES = [C.UFLOAT, C.FLOAT]


def _enc(img, typ, quality):
    return O.encode(img, BC6H, typ=int(typ), quality=quality, threads=16)


def test_half_ints_is_the_oracle_loader_on_every_half():
    """half_ints against the oracle for all 65 536 half patterns, non-finite rows included: a flat block of
    pattern b decodes to half_ints(b).  The oracle agrees on the non-finite rows too (Inf / NaN clamp to 0x7BFF
    under their sign), so nothing had to be settled from the reference, whose compressBlock hands the packed half
    bits to the codec as they are (S3tcConverter.cpp:546-591)."""
    allbits = np.arange(65536, dtype=np.uint16)
    for typ in TYPES:
        for img, g in C.flat_surfaces(allbits):
            got = C.decoded_ints(_enc(img, typ, 0), img, typ)[::4, ::4, 0]
            assert np.array_equal(got, C.half_ints(g, typ == C.FLOAT))


@pytest.mark.parametrize("typ", TYPES)
def test_mode_complete_source_reaches_every_mode(typ):
    src = C.mode_complete_source(typ)
    for q in C.LEVELS:
        C.check_mode_counts(_enc(src, typ, q), q)


def test_mode_of_reads_the_headers_the_source_was_built_from():
    rng = np.random.default_rng(1)
    blocks = rng.integers(0, 256, (14, 8, 16), dtype=np.uint8)
    for m, (bits, val) in C.MODE_HEADERS.items():
        blocks[m - 1, :, 0] = (blocks[m - 1, :, 0] & (0xFF ^ ((1 << bits) - 1))) | val
    assert np.array_equal(C.mode_of(blocks).reshape(14, 8), np.repeat(np.arange(1, 15)[:, None], 8, axis=1))


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("quality", [0, 2, 4])
def test_flat_law(typ, quality):
    C.check_flat_law(_enc, typ, quality)


@pytest.mark.parametrize("typ", TYPES)
def test_byte_law(typ):
    for q in (0, 2):
        C.check_byte_law(_enc, typ, q)


def test_half_boundaries_holds_what_it_says():
    f = C.half_boundaries()
    v = f[..., :3].reshape(-1)
    assert f.shape == (128, 256, 4) and (f[..., 3] == 1).all()
    assert np.isnan(v).sum() == 10 and np.isinf(v).sum() == 2
    h = C.to_half(v[:95229].reshape(-1, 3)).view(np.uint16).astype(np.int64)
    # below the midpoint the lower half, above it the upper one, on it the even one
    k = np.arange(C.MAX_HALF)
    assert np.array_equal(h[:, 0], k) and np.array_equal(h[:, 2], k + 1)
    assert np.array_equal(h[:, 1], k + (k & 1))
    s = C.half_boundaries(True)
    assert np.array_equal(np.abs(s[..., :3][~np.isnan(s[..., :3])]), np.abs(v[~np.isnan(v)]))
    assert 0.4 < np.signbit(s[..., :3]).mean() < 0.6


@pytest.mark.parametrize("typ", TYPES)
def test_float32_law(typ):
    C.check_float32_law(_enc, typ, 1)


@pytest.mark.parametrize("typ", TYPES)
def test_no_block_is_worse_than_the_flat_block(typ):
    """block_error <= flat_bound for every block, every level, every source.  Before the flat candidate
    (id 33) the oracle failed this on 6..7 of 896 mode-complete blocks (UFloat, up to 14 x the bound) and on 3 of
    1024 blocks of the signed probe (Float)."""
    bad = []
    for name, img in C.bound_sources(typ):
        for q in C.LEVELS:
            n, ratio = C.over_flat_bound(_enc(img, typ, q), img, typ)
            if n:
                bad.append("%s level %d: %d blocks, worst %.1f x the flat block" % (name, q, n, ratio))
    assert not bad, "\n".join(bad)
