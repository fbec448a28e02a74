"""The deflate-size estimate's definition (tests/lzsize_ref.py) and the search built on it (tests/rdo_target_ref.py),
without a GPU: the fixed-point logarithm, the code tables, the estimate against zlib at level 9 on real payloads, and
the targets the bisection reaches."""
import math
import zlib

import numpy as np
import pytest

import lzsize_cases as C
import lzsize_ref as Z
import rdo_target_ref


def test_lg16_is_log2_to_16_bits():
    for x in list(range(1, 5001)) + [2**16 - 1, 2**16, 2**16 + 1, 2**31 + 5]:
        got = Z.lg16(x)
        assert abs(got/65536.0 - math.log2(x)) < 1.6e-5, x
        assert got >> 16 == x.bit_length() - 1
    assert Z.lg16(1) == 0 and Z.lg16(2) == 1 << 16 and Z.lg16(1 << 31) == 31 << 16


def test_code_tables_are_rfc_1951():
    assert len(Z.LEN_BASE) == len(Z.LEN_EXTRA) == 29 and len(Z.DIST_BASE) == len(Z.DIST_EXTRA) == 30
    # every base is the one before plus its 2^extra values; length 258 has a code of its own
    for i in range(27):
        assert Z.LEN_BASE[i + 1] == Z.LEN_BASE[i] + (1 << Z.LEN_EXTRA[i])
    assert Z.LEN_BASE[28] == 258 == Z.LEN_BASE[27] + (1 << Z.LEN_EXTRA[27]) - 1
    for i in range(29):
        assert Z.DIST_BASE[i + 1] == Z.DIST_BASE[i] + (1 << Z.DIST_EXTRA[i])
    assert Z.DIST_BASE[29] + (1 << Z.DIST_EXTRA[29]) - 1 == Z.W
    assert [int(Z.length_code(v)) for v in (3, 10, 11, 12, 13, 257, 258)] == [0, 7, 8, 8, 9, 27, 28]
    assert [int(Z.dist_code(v)) for v in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]


def test_the_definition_on_small_streams():
    assert Z.lz_size(b"") == dict.fromkeys(Z.FIELDS, 0)
    one = Z.lz_size(b"x")
    # a literal and the end-of-block symbol: two symbols of one bit each
    assert one == dict(bytes_in=1, bits_q16=2 << 16, est_bytes=1, literals=1, matches=0, matched_bytes=0)
    run = Z.lz_size(np.full(1000, 7, np.uint8))
    assert (run["literals"], run["matches"], run["matched_bytes"]) == (1, 4, 999)
    # spans are their concatenation
    a = np.random.default_rng(0).integers(0, 4, 10000).astype(np.uint8)
    assert Z.lz_size([a[:3333], a[3333:3334], a[3334:]]) == Z.lz_size(a)
    # chunks are independent: no match crosses a multiple of CHUNK
    _, (mp, ml, md) = Z.parse(a)
    assert ((mp % Z.CHUNK) + ml <= Z.CHUNK).all() and (md <= Z.W).all() and (ml >= Z.MIN).all() and (ml <= Z.MAX).all()


@pytest.fixture(scope="module")
def rows():
    return C.payload_rows()


def test_estimate_against_zlib_9(rows):
    assert len(rows) == 2*(10 + 6)
    seen = []
    for name, p in rows:
        z = len(zlib.compress(p.tobytes(), 9))
        est = Z.lz_size(p)["est_bytes"]
        seen.append((name, z, est, est/z))
        print("%-24s zlib-9 %7d  estimate %7d  ratio %.4f" % seen[-1])
    for name, z, est, ratio in seen:
        if z >= 4096:
            assert 0.95 <= ratio <= 1.08, (name, z, est, ratio)
    assert sum(z >= 4096 for _, z, _, _ in seen) == len(seen)


@pytest.mark.parametrize("inp,name", C.TARGET_PAIRS, ids=["%s-%s" % p for p in C.TARGET_PAIRS])
def test_targets(inp, name):
    fmt, typ = C.format_of(name)
    plain, src = C.plain(inp, name), C.inputs()[inp]
    z_plain = len(zlib.compress(plain.tobytes(), 9))
    for target in (0.95, 0.85, 0.70):
        outs, stats, res = rdo_target_ref.rdo_target([plain], [src], fmt, typ, target, 32.0)
        z = len(zlib.compress(outs[0].tobytes(), 9))
        print(inp, name, target, res, "zlib-9 ratio %.4f" % (z/z_plain))
        T = math.floor(float(np.float32(target))*res["est_bytes_plain"])
        assert res["est_bytes_plain"] == Z.lz_size(plain)["est_bytes"]
        assert res["est_bytes_final"] == Z.lz_size(outs[0])["est_bytes"]
        if (inp, name, target) == ("crops", "BC1", 0.70):
            assert (res["reached"], res["lambda16"], res["trials"]) == (0, 512, 1) and res["est_bytes_final"] > T
            continue
        assert res["reached"] == 1 and res["est_bytes_final"] <= T
        assert z/z_plain <= target + 0.02
        # the smallest lambda: one step less misses the target
        if res["lambda16"] > 1:
            less, _ = rdo_target_ref.pass_at([plain], [src], fmt, typ, res["lambda16"] - 1)
            assert Z.lz_size(less)["est_bytes"] > T
        assert stats[0]["blocks_changed"] > 0
