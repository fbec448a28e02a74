"""GPU parity of BC7's first stream trip with its fits' integer statistics handed in (csrc/bc7_encode.hip, "moments handed
in"; csrc/bc7_packed.h: mom_whole, mom_sub): mode 6 and the planes of mode 5 take the block table's moments in their own
channel slots and the extremes of their rotated alpha from the per-block table of channel extremes, the partition lanes
take the subset-1 moments their partition's owner left in LDS and form subset 0 by subtraction.  Every payload must equal
the CPU oracle's byte for byte, at every level with the linear metric and at levels 2..4 with the perceptual one.

The images are the smallest that reach every branch of the new path:
  one / pair / pair_odd     4x4, 8x4, 12x4: the un-paired wave, one pair, a pair plus an odd last block
  alpha_opaque, opaque_alpha  a pair with one alpha-carrying and one opaque half (`any_alpha` beside an opaque half: the
                            constant-255 derivation beside real alpha moments), in both orders
  const_alpha               alpha constant but not 255
  flat, flat_subset         n q - s^2 = 0 in every channel of the block / of one subset (the left two columns: subset 0 of
                            partition 0), the axis left at zero
  ends                      every colour channel reaches 0 and 255 (the extremes table under rotations 1..3)
  photo2                    the 64x64 crop at (144, 96) of synth.photo2(1024, 1024, seed 1): 129 of its 256 blocks take the
                            second pass at Normal and 59 of its 128 pairs hold one block of each kind, so the row-loop trips
                            and the handed-in trip meet in one wave (asserted on the oracle's output below, without a GPU)"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)
CROP_X, CROP_Y = 144, 96


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(7)
    strip = rng.integers(0, 256, (4, 12, 4), dtype=np.uint8)
    strip[..., 3] = 255
    strip[:, 4:8, :3] = (np.arange(16).reshape(4, 4, 1)*np.array([9, 5, 13]) + np.array([20, 90, 10])).astype(np.uint8)   # a ramp
    strip[:, 8:, :3] = np.where((np.arange(4)[:, None] > np.arange(4)[None, :])[..., None], strip[0, 8, :3], strip[3, 11, :3])
    mixed = strip[:, :8].copy()
    mixed[:, :4, 3] = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    mixed[0, 0, 3] = 17
    const_alpha = strip[:, :8].copy()
    const_alpha[..., 3] = 128
    const_alpha[:, 4:, 3] = 1
    flat = np.empty((4, 8, 4), np.uint8)
    flat[:, :4] = (37, 201, 118, 255)
    flat[:, 4:] = (5, 5, 250, 90)
    flat_subset = strip[:, :8].copy()
    flat_subset[:, 0:2, :3] = (200, 30, 99)
    flat_subset[:, 4:6] = (12, 240, 7, 60)
    flat_subset[:, 6:8, 3] = rng.integers(0, 256, (4, 2), dtype=np.uint8)
    ends = rng.integers(1, 255, (4, 8, 4), dtype=np.uint8)
    ends[..., 3] = 255
    ends[:, 4:, 3] = rng.integers(1, 255, (4, 4), dtype=np.uint8)
    for bx in (0, 4):
        for c in range(3):
            ends[c, bx + c, c] = 0
            ends[3 - c, bx + 3 - c, c] = 255
    photo2 = synth.photo2(1024, 1024, seed=1)[CROP_Y:CROP_Y + 64, CROP_X:CROP_X + 64]
    out = {"one": strip[:, :4], "pair": strip[:, :8], "pair_odd": strip, "alpha_opaque": mixed,
           "opaque_alpha": mixed[:, ::-1], "const_alpha": const_alpha, "flat": flat, "flat_subset": flat_subset,
           "ends": ends, "photo2": photo2}
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


NAMES = ("one", "pair", "pair_odd", "alpha_opaque", "opaque_alpha", "const_alpha", "flat", "flat_subset", "ends", "photo2")
CASES = [(q, False) for q in range(5)] + [(q, True) for q in (2, 3, 4)]


@functools.lru_cache(maxsize=None)
def _ref(name, quality, srgb):
    """The oracle's payload of one case: computed once, shared, read-only"""
    ref = O.encode(_images()[name], BC7, quality=quality, threads=8, color_space=1 if srgb else 0)
    ref.setflags(write=False)
    return ref


def _mode_numbers(payload):
    """The mode of every block: the position of the lowest set bit of its first byte"""
    first = payload.reshape(-1, 16)[:, 0].astype(np.int64) | 256
    return np.array([int(v & -v).bit_length() - 1 for v in first])


# ---- what the images are: conditions on the images and on the oracle's output alone (no GPU) ----

def test_images_are_what_they_say():
    im = _images()
    assert [im[k].shape[:2] for k in ("one", "pair", "pair_odd")] == [(4, 4), (4, 8), (4, 12)]
    a = im["alpha_opaque"]
    assert (a[:, :4, 3] != 255).any() and (a[:, 4:, 3] == 255).all()
    assert (im["opaque_alpha"][:, :4, 3] == 255).all() and (im["opaque_alpha"][:, 4:, 3] != 255).any()
    c = im["const_alpha"]
    assert len(np.unique(c[:, :4, 3])) == 1 and len(np.unique(c[:, 4:, 3])) == 1 and (c[..., 3] != 255).all()
    f = im["flat"]
    assert len(np.unique(f[:, :4].reshape(-1, 4), axis=0)) == 1 and len(np.unique(f[:, 4:].reshape(-1, 4), axis=0)) == 1
    s = im["flat_subset"]
    assert len(np.unique(s[:, 0:2].reshape(-1, 4), axis=0)) == 1 and len(np.unique(s[:, 2:4].reshape(-1, 4), axis=0)) > 1
    assert len(np.unique(s[:, 4:6].reshape(-1, 4), axis=0)) == 1 and len(np.unique(s[:, 6:8].reshape(-1, 4), axis=0)) > 1
    e = im["ends"]
    for bx in (0, 4):
        blk = e[:, bx:bx + 4, :3].reshape(16, 3)
        assert (blk.min(axis=0) == 0).all() and (blk.max(axis=0) == 255).all()


def test_photo2_crop_has_blocks_of_both_kinds_in_one_wave():
    """Blocks whose Normal payload is mode 0, 2 or 4 took the second pass; a pair is two neighbouring blocks of a row"""
    second = np.isin(_mode_numbers(_ref("photo2", 2, False)), (0, 2, 4)).reshape(16, 16)
    assert 64 < second.sum() < 192, second.sum()
    assert (second[:, 0::2] != second[:, 1::2]).sum() >= 32


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
