"""GPU parity of BC7 with the candidate word stored beside each candidate (csrc/bc7_cand.h; csrc/bc7_encode.hip: `take`,
the starts trip, the perturbation pass): every payload must equal the CPU oracle's byte for byte, at every level with
the linear metric and at levels 2..4 with the perceptual one.

What a stored candidate is now travels with it, and a fit's texels come from one table per (subsets, partition, fit): the
images make every mode win, on many partitions, so that every shape of the word and every row of the table is
exercised, through to the packed block.  Their blocks come from seeded
generators (what the blocks turn out to be is asserted below, on the oracle's output alone):
  three(seed)   three colours in 2x2 quarters, one texel moved, a little noise: modes 1, 2, 3 (tests/test_gpu_bc7_lane_roles.py)
  grad3(seed)   three colour gradients laid out by one of the first 16 three-subset partitions: modes 0 and 2
  alpha4(seed)  a colour line with independent random alpha: mode 4 (tests/test_gpu_bc7_lane_roles.py)
  two7(seed)    two colours with their own alpha laid out by a two-subset partition, a little noise: modes 7, 5, 6
  one / pair / pair_odd   4x4, 8x4, 12x4: the un-paired wave, one pair, a pair plus an odd last block
  opaque        64x48: 96 three blocks, 96 grad3 blocks
  mixed         64x64: blocks with alpha (alpha4, two7) and without (three, grad3) alternate along every row, rows starting
                with either kind: in the 32-lane layouts two neighbouring blocks share a wave, in both orders
  photo2        the 64x64 crop at (144, 96) of synth.photo2(1024, 1024, seed 1)"""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth
from test_bc7_cand_words import PART2, PART3

BC7 = int(Format.BC7)
CROP_X, CROP_Y = 144, 96


def three(seed):
    r = np.random.default_rng(seed)
    cols = r.integers(0, 256, (3, 3))
    lab = r.integers(0, 3, (2, 2)).repeat(2, 0).repeat(2, 1)
    lab[r.integers(0, 4), r.integers(0, 4)] = r.integers(0, 3)
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(cols[lab] + r.integers(-6, 7, (4, 4, 3)), 0, 255)
    b[..., 3] = 255
    return b


def alpha4(seed):
    r = np.random.default_rng(seed)
    c0, c1 = r.integers(0, 256, 3), r.integers(0, 256, 3)
    t = r.random((4, 4, 1))
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(c0 + (c1 - c0)*t + r.integers(-3, 4, (4, 4, 3)), 0, 255)
    b[..., 3] = r.integers(0, 255, (4, 4))
    return b


def grad3(seed):
    r = np.random.default_rng(2000 + seed)
    p = PART3[int(r.integers(0, 16))]
    lab = np.array([(p >> (2*t)) & 3 for t in range(16)]).reshape(4, 4)
    c0 = r.integers(0, 256, (3, 3))
    c1 = np.clip(c0 + r.integers(-60, 61, (3, 3)), 0, 255)
    t = r.random((4, 4, 1))
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(np.rint(c0[lab] + (c1[lab] - c0[lab])*t), 0, 255)
    b[..., 3] = 255
    return b


def two7(seed):
    r = np.random.default_rng(1000 + seed)
    p = PART2[int(r.integers(0, 64))]
    lab = np.array([(p >> t) & 1 for t in range(16)]).reshape(4, 4)
    cols = r.integers(0, 256, (2, 4))
    cols[:, 3] = r.integers(0, 240, 2)          # per-subset alpha, never opaque
    return np.clip(cols[lab] + r.integers(-3, 4, (4, 4, 4)), 0, 255).astype(np.uint8)


def _grid(blocks, per_row):
    rows = [np.concatenate(blocks[i:i + per_row], axis=1) for i in range(0, len(blocks), per_row)]
    return np.concatenate(rows, axis=0)


@functools.lru_cache(maxsize=None)
def _images():
    strip = np.concatenate([grad3(0), three(0), two7(1)], axis=1)
    opaque = _grid([three(s) for s in range(96)] + [grad3(s) for s in range(96)], 16)
    # 16 rows of 16 blocks; row y, column x: with alpha when x + y is even
    withs = [alpha4(s) for s in range(64)] + [two7(s) for s in range(64)]
    withouts = [three(100 + s) for s in range(64)] + [grad3(100 + s) for s in range(64)]
    mixed = _grid([(withs if (x + y) % 2 == 0 else withouts)[(y*16 + x)//2] for y in range(16) for x in range(16)], 16)
    out = {"one": strip[:, :4], "pair": strip[:, :8], "pair_odd": strip, "opaque": opaque, "mixed": mixed,
           "photo2": synth.photo2(1024, 1024, seed=1)[CROP_Y:CROP_Y + 64, CROP_X:CROP_X + 64]}
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


NAMES = ("one", "pair", "pair_odd", "opaque", "mixed", "photo2")
CASES = [(q, False) for q in range(5)] + [(q, True) for q in (2, 3, 4)]


@functools.lru_cache(maxsize=None)
def _ref(name, quality, srgb):
    """The oracle's payload of one case: computed once, shared, read-only"""
    ref = O.encode(_images()[name], BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return ref


def _winners(payload):
    """(mode, partition) of every block: the mode is the position of the lowest set bit, the partition follows it"""
    out = []
    for blk in payload.reshape(-1, 16):
        v = int(blk[0]) | (int(blk[1]) << 8) | (int(blk[2]) << 16)
        mode = ((v | 256) & -(v | 256)).bit_length() - 1
        pbits = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}.get(mode, 0)
        out.append((mode, (v >> (mode + 1)) & ((1 << pbits) - 1)))
    return out


# ---- what the images are: conditions on the images and on the oracle's output alone (no GPU) ----

def test_images_are_what_they_say():
    im = _images()
    assert [im[k].shape[:2] for k in ("one", "pair", "pair_odd")] == [(4, 4), (4, 8), (4, 12)]
    assert all(v.shape[0] <= 64 and v.shape[1] <= 64 for v in im.values())
    # blocks with and without alpha share a wave (blocks 2 k, 2 k + 1 of a row) in both orders
    a = (im["mixed"][..., 3] != 255).reshape(16, 4, 16, 4).any(axis=(1, 3))
    pairs = set(zip(a[:, 0::2].ravel().tolist(), a[:, 1::2].ravel().tolist()))
    assert {(True, False), (False, True)} <= pairs


# the modes a level's search reaches (csrc/bc7_encode.hip, "fit streams"): Lowest mode 6 and, with alpha, mode 5; Low
# the first pass of Normal's layout; from Normal on every mode
REACHED = {0: (5, 6), 1: (1, 3, 5, 6, 7), 2: range(8), 3: range(8), 4: range(8)}


@pytest.mark.parametrize("quality", range(5))
def test_every_mode_wins_blocks(quality):
    wins = collections.Counter(m for name in NAMES for m, _ in _winners(_ref(name, quality, False)))
    for mode in REACHED[quality]:
        assert wins[mode] >= 8, (quality, mode, sorted(wins.items()))


@pytest.mark.parametrize("quality", (2, 3, 4))
def test_many_partitions_win(quality):
    won = [w for name in NAMES for w in _winners(_ref(name, quality, False))]
    assert len({p for m, p in won if m in (1, 3, 7)}) >= 16
    assert len({p for m, p in won if m in (0, 2)}) >= 8


# ---- parity ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, name, quality, srgb):
    img, ref = _images()[name], _ref(name, quality, srgb)
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    got = gpu_ctx.encode([img], make_params(Format.BC7, Type.UNorm, quality, **kw))[0]
    assert got.size == ref.size == (img.shape[0]//4)*(img.shape[1]//4)*16
    bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
    assert bad.size == 0, "%d blocks differ: %s" % (bad.size, bad[:10])
