"""tests/rdo2d_ref.py, the definition of the rate-distortion pass with copies from the block row above, on the CPU:
where it must equal the plain pass, the independence of tiles, the window, BC7's reserved mode, and the deflate-9
size on the six photo crops."""
import os
import zlib

import numpy as np
import pytest

import oracle_lib
import rdo2d_ref
import rdo_ref
from cuttlefish_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = sorted(rdo_ref.TABLE)
SEG, R = rdo_ref.SEG, rdo2d_ref.TILE_ROWS
LAM = 8.0


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


@pytest.fixture(scope="module")
def surfaces():
    """{(fmt, typ): (source, plain payload)}: SEG + 3 blocks wide (two tiles a row, one partial), 2 R + 1 block rows"""
    out = {}
    for fmt, typ in ROWS:
        src = synth.photo(4*(SEG + 3) - 1, 4*(2*R + 1) - 2, seed=fmt)
        out[(fmt, typ)] = (src, oracle_lib.encode(src, fmt, typ, 1))
    return out


@pytest.mark.parametrize("fmt,typ", ROWS)
def test_without_row_above_it_is_the_plain_pass(surfaces, fmt, typ):
    src, plain = surfaces[(fmt, typ)]
    want = rdo_ref.rdo(plain, src, fmt, typ, LAM, max_sse_increase=300)
    assert _same(rdo2d_ref.rdo2d(plain, src, fmt, typ, LAM, 300, (True,)*4, False), want)
    # tiles of one row have no row above: the tiled walk itself is the plain pass
    assert _same(rdo2d_ref.rdo2d(plain, src, fmt, typ, LAM, 300, (True,)*4, True, tile_rows=1), want)
    # and with it something changes
    got = rdo2d_ref.rdo2d(plain, src, fmt, typ, LAM, 300, (True,)*4, True)
    assert not np.array_equal(got[0], want[0])
    assert got[1]["blocks"] == want[1]["blocks"] and got[1]["sse_before"] == want[1]["sse_before"]


@pytest.mark.parametrize("fmt", [rdo_ref.BC1_RGB, rdo_ref.BC3, rdo_ref.BC7])
def test_tiles_are_independent(fmt):
    bs = rdo_ref.TABLE[(fmt, 0)][0]
    bx = SEG + 5
    src = synth.photo(4*bx, 4*2*R, seed=11)
    plain = oracle_lib.encode(src, fmt, 0, 1)
    full, st = rdo2d_ref.rdo2d(plain, src, fmt, 0, LAM, None, (True,)*4, True)
    halves = [rdo2d_ref.rdo2d(plain[k*R*bx*bs:(k + 1)*R*bx*bs], src[4*R*k:4*R*(k + 1)], fmt, 0, LAM, None, (True,)*4, True)
              for k in range(2)]
    assert np.array_equal(full, np.concatenate([o for o, _ in halves]))
    assert st == {k: halves[0][1][k] + halves[1][1][k] for k in st}
    # the first row of a tile copies from its left only
    left, _ = rdo_ref.rdo(plain, src, fmt, 0, LAM)
    full, left = full.reshape(2*R, bx, bs), left.reshape(2*R, bx, bs)
    assert np.array_equal(full[0], left[0]) and np.array_equal(full[R], left[R])
    assert not np.array_equal(full[1:R], left[1:R])
    # tiles are SEG blocks wide: the first block of the second tile of a row copies from above only
    whole, _ = rdo2d_ref.rdo2d(plain, src, fmt, 0, LAM, None, (True,)*4, True, seg=0)
    assert not np.array_equal(whole.reshape(2*R, bx, bs)[:, SEG:], full[:, SEG:])
    assert np.array_equal(full[0, SEG], plain.reshape(2*R, bx, bs)[0, SEG])


@pytest.mark.parametrize("fmt,typ", ROWS)
def test_a_small_window_gives_the_plain_pass(surfaces, fmt, typ):
    src, plain = surfaces[(fmt, typ)]
    bs = rdo_ref.TABLE[(fmt, typ)][0]
    bx = (src.shape[1] + 3)//4
    want = rdo_ref.rdo(plain, src, fmt, typ, LAM)
    edge = (bx + rdo2d_ref.UP//2)*bs
    assert _same(rdo2d_ref.rdo2d(plain, src, fmt, typ, LAM, None, (True,)*4, True, window_bytes=edge - 1), want)
    assert not _same(rdo2d_ref.rdo2d(plain, src, fmt, typ, LAM, None, (True,)*4, True, window_bytes=edge), want)
    assert not rdo2d_ref.has_up(bx, bs, False) and rdo2d_ref.has_up(bx, bs, True)
    # deflate's window holds the row above up to 4092 blocks of 8 bytes, 2044 of 16
    assert rdo2d_ref.has_up(4096 - 4, 8, True) and not rdo2d_ref.has_up(4096 - 3, 8, True)


def test_no_bc7_block_is_in_the_reserved_mode():
    # flat areas make byte 0 of many blocks equal; a splice of the low half of a block whose mode bit sits higher
    # would give byte 0 == 0
    src = synth.photo(4*(SEG + 3), 4*(R + 2), seed=5)
    plain = oracle_lib.encode(src, rdo_ref.BC7, 0, 1)
    assert plain.reshape(-1, 16)[:, 0].all()
    for lam in (4.0, 256.0):
        out, st = rdo2d_ref.rdo2d(plain, src, rdo_ref.BC7, 0, lam, None, (False,)*4, True)
        assert out.reshape(-1, 16)[:, 0].all() and st["blocks_changed"] > 0


def test_rates_and_candidate_numbers():
    # a block of the row above at dx = 0 lies bx blocks back; to its left, further back
    assert rdo2d_ref.rate_up(8, 8, 1024, 0) == 12 + 2*13 and rdo2d_ref.rate_up(8, 8, 1024, -1) == 12 + 2*13
    assert rdo2d_ref.rate_up(8, 8, 1024, 1) == 12 + 2*12 and rdo2d_ref.rate_up(16, 8, 5, 3) == 64 + 12 + 2*5
    for (fmt, typ), n in zip(ROWS, (73, 73, 97, 169, 73, 169, 73)):
        assert 1 + (rdo_ref.L + rdo2d_ref.UP)*len(rdo_ref.TABLE[(fmt, typ)][2]) == n


def test_deflate_size_falls_below_the_plain_pass_on_the_crops():
    crops = np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]
    src = np.ascontiguousarray(np.concatenate(list(crops), axis=1))
    plain = oracle_lib.encode(src, rdo_ref.BC1_RGB, 0, 2)
    sizes = [len(zlib.compress(p.tobytes(), 9)) for p in (
        plain, rdo_ref.rdo(plain, src, rdo_ref.BC1_RGB, 0, 4.0)[0],
        rdo2d_ref.rdo2d(plain, src, rdo_ref.BC1_RGB, 0, 4.0, None, (True,)*4, True)[0])]
    print("BC1_RGB lambda 4, six crops side by side: plain %d, left only %d, with the row above %d" % tuple(sizes))
    assert sizes[2] < sizes[1] < sizes[0]
