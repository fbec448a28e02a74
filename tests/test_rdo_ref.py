"""tests/rdo_ref.py, the definition of the rate-distortion pass, on the CPU: the per-block error cap, the independence
of segments, the deflate-9 size on the six photo crops, and the statistics against an independent measurement."""
import os
import zlib

import numpy as np
import pytest

import oracle_lib
import rdo_ref
from cuttlefish_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (1, 3, 8)


def _block_sse(payload, src, fmt, chans):
    """per-block SSE of a payload against an RGBA8 source, by a whole-surface decode: (by, bx) int64"""
    h, w = src.shape[:2]
    dec = oracle_lib.decode(payload, fmt, w, h).astype(np.int64)
    d = (dec - src.astype(np.int64))[..., list(chans)]
    e = np.zeros((4*((h + 3)//4), 4*((w + 3)//4)), np.int64)
    e[:h, :w] = (d*d).sum(axis=2)
    return e.reshape(e.shape[0]//4, 4, e.shape[1]//4, 4).sum(axis=(1, 3))


@pytest.fixture(scope="module")
def crops():
    return [np.ascontiguousarray(c) for c in np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]]


@pytest.fixture(scope="module")
def crop_runs(crops):
    """{fmt: (plain payloads, {lambda: [(payload, stats) per crop]})} for BC1_RGB and BC7 Normal"""
    runs = {}
    for fmt in (rdo_ref.BC1_RGB, rdo_ref.BC7):
        plain = [oracle_lib.encode(c, fmt, 0, 2) for c in crops]
        runs[fmt] = (plain, {lam: [rdo_ref.rdo(p, c, fmt, 0, lam) for p, c in zip(plain, crops)] for lam in LAMBDAS})
    return runs


def _deflated(payloads):
    return sum(len(zlib.compress(p.tobytes(), 9)) for p in payloads)


@pytest.mark.parametrize("fmt", [rdo_ref.BC1_RGB, rdo_ref.BC7])
def test_pooled_deflate_size_falls_on_the_crops(crop_runs, fmt):
    plain, by_lambda = crop_runs[fmt]
    sizes = [_deflated([o for o, _ in by_lambda[lam]]) for lam in LAMBDAS]
    print("format %d: plain %d, lambda 1 / 3 / 8: %r" % (fmt, _deflated(plain), sizes))
    assert sizes[1] < _deflated(plain)
    assert sizes[0] >= sizes[1] >= sizes[2]


@pytest.mark.parametrize("fmt", [rdo_ref.BC1_RGB, rdo_ref.BC7])
def test_stats_equal_an_independent_decode_and_subtract(crops, crop_runs, fmt):
    plain, by_lambda = crop_runs[fmt]
    chans = rdo_ref.TABLE[(fmt, 0)][1]
    for p, c, (o, st) in zip(plain, crops, by_lambda[3]):
        assert st["sse_before"] == int(_block_sse(p, c, fmt, chans).sum())
        assert st["sse_after"] == int(_block_sse(o, c, fmt, chans).sum())
        bs = rdo_ref.TABLE[(fmt, 0)][0]
        assert st["blocks"] == 32*32 and st["bits_before"] == 32*32*8*bs and st["bits_after"] <= st["bits_before"]
        assert st["blocks_changed"] == int((o.reshape(-1, bs) != p.reshape(-1, bs)).any(axis=1).sum()) > 0


@pytest.mark.parametrize("fmt", sorted(f for f, _ in rdo_ref.TABLE))
@pytest.mark.parametrize("cap", [0, 37, 5000])
def test_no_block_exceeds_its_cap(fmt, cap):
    src = synth.photo(4*(rdo_ref.L + 9) - 2, 11, seed=fmt)
    mask = (True, True, False, True)
    plain = oracle_lib.encode(src, fmt, 0, 1)
    out, st = rdo_ref.rdo(plain, src, fmt, 0, 16.0, max_sse_increase=cap, mask=mask)
    chans = [c for c in rdo_ref.TABLE[(fmt, 0)][1] if mask[c]]
    before, after = _block_sse(plain, src, fmt, chans), _block_sse(out, src, fmt, chans)
    assert (after <= before + cap).all()
    assert (st["sse_before"], st["sse_after"]) == (int(before.sum()), int(after.sum()))
    if cap == 5000:
        assert st["blocks_changed"] > 0 and (after > before).any()


def test_uncapped_pass_may_exceed_what_a_cap_allows():
    src = synth.photo(128, 16, seed=3)
    plain = oracle_lib.encode(src, rdo_ref.BC7, 0, 1)
    free, _ = rdo_ref.rdo(plain, src, rdo_ref.BC7, 0, 64.0)
    chans = (0, 1, 2, 3)
    assert (_block_sse(free, src, rdo_ref.BC7, chans) > _block_sse(plain, src, rdo_ref.BC7, chans) + 37).any()


@pytest.mark.parametrize("fmt", [rdo_ref.BC1_RGBA, rdo_ref.BC3, rdo_ref.BC7])
def test_segments_are_independent(fmt):
    seg, bs = rdo_ref.SEG, rdo_ref.TABLE[(fmt, 0)][0]
    bx = 2*seg + 5
    src = synth.photo(4*bx, 12, seed=7)
    plain = oracle_lib.encode(src, fmt, 0, 1)
    full, _ = rdo_ref.rdo(plain, src, fmt, 0, 8.0)
    full, plain = full.reshape(3, bx, bs), plain.reshape(3, bx, bs)
    changed = 0
    for row in range(3):
        for k in range(3):
            x0, x1 = k*seg, min((k + 1)*seg, bx)
            part, _ = rdo_ref.rdo(plain[row, x0:x1].reshape(-1), src[4*row:4*row + 4, 4*x0:4*x1], fmt, 0, 8.0)
            assert np.array_equal(part.reshape(-1, bs), full[row, x0:x1]), (row, k)
            # the first block of a segment has nothing to copy from
            assert np.array_equal(full[row, x0], plain[row, x0])
            changed += int((part.reshape(-1, bs) != plain[row, x0:x1]).any(axis=1).sum())
    assert changed > 0


def test_rate_model_and_quantiser():
    assert rdo_ref.rate(8, 8, 1) == 12 + 2*3 and rdo_ref.rate(16, 8, 16) == 64 + 12 + 2*8
    assert rdo_ref.rate(16, 2, 3) == 8*14 + 12 + 2*5
    assert rdo_ref.lambda16(3) == 48 and rdo_ref.lambda16(0.03) == 0 and rdo_ref.lambda16(1024) == 16384
    for bad in (0, -1, 1024.5, float("nan")):
        with pytest.raises(ValueError):
            rdo_ref.lambda16(bad)
    f = np.array([[[-1.0, 0.6/255, 1.4/255, 2.0], [np.nan, 0.4/255, 254.6/255, 1.0]]], np.float32)
    assert rdo_ref.quantise(f).tolist() == [[[0, 1, 1, 255], [0, 0, 255, 255]]]
    assert rdo_ref.quantise(f.astype(np.float16)).dtype == np.uint8
