"""The ASTC cases of tests/astc_cases.py held for the oracle alone (no GPU): the partition hash and the block parser
against the independent decoder, the census of what each source makes win as conditions, and the launch shapes of the
kernel's plan.  Run with -s for the census tables (DESIGN.md 4.5 holds a copy)."""
import collections
import ctypes

import numpy as np
import pytest

import astc_cases as C
import oracle_lib as O

ALL_KEYS = C.PAINTED4 + C.PAINTED3 + C.PLAIN


def _name(fmt):
    return "%dx%d" % C.FOOT[fmt]


def test_select_partition_is_the_decoders():
    L = O.lib()
    for bw, bh in ((4, 4), (5, 4), (6, 6), (8, 5), (12, 12)):
        for parts in (2, 3, 4):
            for seed in range(0, 1024, 5):
                want = [[L.astc_select_partition(seed, x, y, parts, 1 if bw*bh < 31 else 0) for x in range(bw)]
                        for y in range(bh)]
                assert np.array_equal(C.select_partition(seed, bw, bh, parts), want), (bw, bh, parts, seed)


def test_colour_unquantisation_spans_the_byte_range():
    """every colour range unquantises to distinct values from 0 to 255 (the law below pins the values themselves to
    the decoder); sizes of a few integer sequences from the specification's formula"""
    for q in C.CQ:
        vals = sorted(C.unquant_colour(q, v) for v in range(q[0]))
        assert len(set(vals)) == q[0] and vals[0] == 0 and vals[-1] == 255, q
    assert [C.ise_bits(n, q) for n, q in ((8, C.CQ[0]), (5, C.WQ[1]), (3, C.WQ[3]), (18, C.CQ[16]))] == [21, 8, 7, 144]


@pytest.mark.parametrize("fmt", C.FORMATS, ids=_name)
def test_parser_agrees_with_the_decoder_on_every_block(fmt):
    """the law of astc_cases.check_endpoint_law over every payload the census is taken from"""
    checked = 0
    for key in ALL_KEYS:
        img = C.source(key, fmt)
        for q in C.levels_of(key):
            checked += C.check_endpoint_law(C.ref(key, fmt, q), fmt, img.shape[1], img.shape[0])
    assert checked > 1500


@pytest.mark.parametrize("fmt", C.FORMATS, ids=_name)
def test_census_of_the_oracle(fmt):
    total = {k: collections.Counter() for k in ("parts", "cem", "cem_multi", "ccs", "wlevels", "clevels", "contracted")}
    void = 0
    print()
    for key in ALL_KEYS:
        for q in C.levels_of(key):
            c = C.check_census(key, fmt, q, C.ref(key, fmt, q))
            for k in total:
                total[k] += c[k]
            void += c["void"]
            print("%-6s %-26s Q%d  %s" % (_name(fmt), " ".join(str(k) for k in key), q, C.census_line(c)))
    total["void"] = void
    print("%-6s all sources: %s; contraction %s" % (_name(fmt), C.census_line(total), dict(total["contracted"])))
    # direct endpoints, with and without alpha, with and without blue contraction
    assert total["cem"][8] and total["cem"][12]
    for cem in (8, 12):
        assert total["contracted"][(cem, True)] and total["contracted"][(cem, False)], cem
    # base + offset is searched on the two smallest footprints only
    if fmt in (43, 44):
        assert total["cem"][9] and total["cem"][13]
    else:
        assert not total["cem"][9] and not total["cem"][13]
    assert set(total["cem"]) <= {0, 4, 6, 8, 9, 10, 12, 13}
    # a second plane on each of the four channels
    assert all(total["ccs"][k] for k in range(4)), total["ccs"]
    # every weight range some legal grid of the footprint can carry
    assert set(total["wlevels"]) == C.legal_weight_levels(*C.FOOT[fmt]), sorted(total["wlevels"])
    assert set(C.WLEVELS) == C.legal_weight_levels(*C.FOOT[fmt])
    assert len(total["clevels"]) >= 8 and max(total["clevels"]) == 256, total["clevels"]


def test_colour_ranges_over_all_footprints():
    """the colour ranges seen: from the packer's lowest (10 levels, on multi-partition blocks; one partition stops at
    16: minlv of the config lists) to its highest"""
    seen = collections.Counter()
    for fmt in C.FORMATS:
        for key in ALL_KEYS:
            for q in C.levels_of(key):
                seen += C.census(C.ref(key, fmt, q), fmt)["clevels"]
    print("\ncolour ranges: %s" % sorted(seen.items()))
    assert len(seen) >= 8 and min(seen) == 10 and max(seen) == 256, seen


@pytest.mark.parametrize("fmt", C.FORMATS, ids=_name)
def test_four_partitions_with_alpha_stay_legal(fmt):
    """four partitions with alpha are out of the format's reach (4 x 6 values and more): the blocks stay legal, and
    the wider search of Highest has the lower mean error -- in the metric the encoder minimises, which is the plain
    RGBA error under Alpha::Encoded (under Alpha::Standard the texel's alpha weighs its colour error)"""
    key = ("painted", 4, "alpha")
    img = C.source(key, fmt).astype(np.int64)
    err = []
    for q in (C.NORMAL, C.HIGHEST):
        _, bad = O.decode_astc(C.ref(key, fmt, q), fmt, img.shape[1], img.shape[0])               # Alpha::Standard
        assert bad == 0
        dec, bad = O.decode_astc(C.ref(key, fmt, q, alpha=3), fmt, img.shape[1], img.shape[0])    # Alpha::Encoded
        assert bad == 0
        err.append(float(((dec - img)**2).mean()))
    assert err[1] < err[0], err


def test_void_extent_float_source_is_not_on_the_byte_grid():
    """the float form holds values between two bytes, outside 0..1 and beside a rounding tie"""
    f = C.void_extent_f32(6, 6)
    assert (f > 1).any() and (f < 0).any()
    assert (np.abs(f*255 - np.round(f*255)) > 0.2).any()
    solid, _ = C.solid_blocks(f, 47)
    assert solid.sum() >= 12


# ---- HDR profiles ----------------------------------------------------------------------------------------------

# source alpha -> Alpha::None (reads 1), PreMultiplied (HDR RGB with LDR alpha), Standard (HDR RGBA)
HDR_ALPHAS = C.HDR_ALPHAS


def hdr_census(payload, fmt):
    parts, cems = collections.Counter(), collections.Counter()
    bad = 0
    for b in C.parse_payload(payload, fmt):
        if b is None:
            bad += 1
        elif not b.void:
            parts[b.parts] += 1
            cems[b.cems[0]] += 1
    return parts, cems, bad


@pytest.mark.parametrize("fmt", C.HDR_FORMATS, ids=_name)
def test_hdr_census_of_the_oracle(fmt):
    """Measured on the oracle (all levels, both alpha profiles, painted with 2, 3 and 4 partitions): partition counts
    1, 2 and 3 and the endpoint modes 7 and 11 (opaque), 14 (LDR alpha) and 15 (HDR alpha) win on at least three
    blocks at every footprint.  Out of reach on this content: four partitions (4 x 8 values of mode 11 do not fit
    18, and the HDR search proposes none), and the luminance modes 2 and 3 (the content is coloured;
    test_gpu_astc_hdr.py holds them on grey content)."""
    parts, cems = collections.Counter(), collections.Counter()
    print()
    for P in (2, 3, 4):
        for alpha in ("one", "ldr", "hdr"):
            key = ("hdr_painted", P, alpha)
            img = C.source(key, fmt)
            for q in range(5):
                pay = C.ref(key, fmt, q, typ=C.UFLOAT, alpha=HDR_ALPHAS[alpha])
                p, c, bad = hdr_census(pay, fmt)
                assert bad == 0
                _, undecoded = O.decode_astc_hdr(pay, fmt, img.shape[1], img.shape[0])
                assert undecoded == 0
                assert set(c) <= set(C.HDR_CEMS), c
                parts += p
                cems += c
                print("%-6s hdr painted P%d alpha %-3s Q%d  P%s cem%s" % (_name(fmt), P, alpha, q, dict(p), dict(c)))
    print("%-6s HDR all: P%s cem%s" % (_name(fmt), dict(parts), dict(cems)))
    assert all(parts[p] >= 3 for p in C.HDR_REACHED_PARTS), parts
    assert all(cems[c] >= 3 for c in C.HDR_REACHED_CEMS), cems


# ---- launch shapes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hdr", [False, True], ids=["ldr", "hdr"])
@pytest.mark.parametrize("quality", C.SHAPE_LEVELS)
@pytest.mark.parametrize("fmt", C.SHAPE_FORMATS, ids=_name)
def test_launch_sweep_reaches_every_shape_of_the_plan(hip_lib, fmt, quality, hdr):
    """(waves per workgroup, 168-register build, blocks a wave searches at a time) for 1..100 blocks per row, from the
    library's own plan with 160 KB of LDS per compute unit: the shapes are the ones astc_cases.SWEEP names, and its
    widths select every one of them -- with a full last workgroup and with the raggedest one the plan allows."""
    shapes, widths = C.SWEEP[(fmt, quality, hdr)]
    picks, made = C.sweep_widths(hip_lib, fmt, quality, hdr)
    print("\n%-6s Q%d %s: %s" % (_name(fmt), quality, "HDR" if hdr else "LDR", " ".join(
        "%dw%s%s@%s" % (s[0], "/168" if s[1] else "/256", "/2" if s[2] == 2 else "/1", list(picks[s])) for s in sorted(picks))))
    assert sorted(picks) == shapes
    assert made == widths
    reached = collections.defaultdict(list)
    for bx in widths:
        reached[C.launch_shape(hip_lib, fmt, quality, hdr, bx)].append(bx)
    assert sorted(reached) == shapes
    for shape, bxs in reached.items():
        per = shape[0]*4
        assert any(b % per == 0 for b in bxs), (shape, bxs)             # a full last workgroup
        assert shape[2] == (2 if quality <= C.NORMAL else 1) and not (hdr and shape[1])
        if picks[shape][1]:                                                 # full workgroups, then a partial one
            assert picks[shape][1] in bxs and picks[shape][1] > per and picks[shape][1] % per
    assert {1, 2, 3} <= set(widths) and max(widths) > 48
