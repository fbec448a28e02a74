"""GPU parity of BC7 with the lane roles read from the packed role / fit words (csrc/bc7_roles.h; csrc/bc7_encode.hip,
"lane roles" and "assemble candidates"): every payload must equal the CPU oracle's byte for byte, at every level with the
linear metric and at levels 2..4 with the perceptual one.

The images are the smallest that reach every row of the role table.  Their blocks come from two seeded generators, and
the seeds were found by a search with the oracle on the CPU (what the blocks are is asserted below, on the oracle's
output alone):
  three(seed)   three colours in 2x2 quarters, one texel moved, a little noise: an opaque block that the three-subset
                modes win at Normal -- seed 0 mode 2, seed 45 mode 0 -- so it walked the second pass
  alpha4(seed)  a colour line with independent random alpha: mode 4 wins at Normal, the second pass of an alpha-carrying half
  flat          one colour: coded exactly by the first pass, which ends its search
  one / pair / pair_odd   4x4, 8x4, 12x4: the un-paired wave whose upper 32 lanes hold no slot, one pair, a pair plus an
                          odd last block
  alpha_opaque, opaque_alpha   alpha4 beside three, in both orders: an alpha-carrying and an opaque half, both walking the
                          second pass -- mode-4 planes in lanes 11 + 2 k / 12 + 2 k beside three-subset slots in the odd
                          lanes from 11 and subset 2 in lane s
  gated_flat, flat_gated  three beside flat, in both orders: exactly one half walks the second pass
  mode0_alpha             the mode-0 block beside another alpha4 block
  photo2                  the 64x64 crop at (144, 96) of synth.photo2(1024, 1024, seed 1), which mixes both kinds of block
                          inside waves (tests/test_gpu_bc7_stream_moments.py)"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

BC7 = int(Format.BC7)
CROP_X, CROP_Y = 144, 96
SEED_MODE2, SEED_MODE0, SEED_ALPHA, SEED_ALPHA_B = 0, 45, 0, 1


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


@functools.lru_cache(maxsize=None)
def _images():
    flat = np.empty((4, 4, 4), np.uint8)
    flat[:] = (37, 201, 118, 255)
    t2, t0, a4, a4b = three(SEED_MODE2), three(SEED_MODE0), alpha4(SEED_ALPHA), alpha4(SEED_ALPHA_B)
    strip = np.concatenate([t2, t0, three(2)], axis=1)
    out = {"one": strip[:, :4], "pair": strip[:, :8], "pair_odd": strip,
           "alpha_opaque": np.concatenate([a4, t2], axis=1), "opaque_alpha": np.concatenate([t2, a4], axis=1),
           "gated_flat": np.concatenate([t2, flat], axis=1), "flat_gated": np.concatenate([flat, t0], axis=1),
           "mode0_alpha": np.concatenate([t0, a4b], axis=1),
           "photo2": synth.photo2(1024, 1024, seed=1)[CROP_Y:CROP_Y + 64, CROP_X:CROP_X + 64]}
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


NAMES = ("one", "pair", "pair_odd", "alpha_opaque", "opaque_alpha", "gated_flat", "flat_gated", "mode0_alpha", "photo2")
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
    return [int(v & -v).bit_length() - 1 for v in first]


# ---- what the images are: conditions on the images and on the oracle's output alone (no GPU) ----

def test_images_are_what_they_say():
    im = _images()
    assert [im[k].shape[:2] for k in ("one", "pair", "pair_odd")] == [(4, 4), (4, 8), (4, 12)]
    # the three-subset modes and mode 4 win in the halves meant to reach them (Normal, linear metric)
    assert _mode_numbers(_ref("pair", 2, False)) == [2, 0]
    assert _mode_numbers(_ref("alpha_opaque", 2, False)) == [4, 2]
    assert _mode_numbers(_ref("opaque_alpha", 2, False)) == [2, 4]
    assert _mode_numbers(_ref("mode0_alpha", 2, False)) == [0, 4]
    a = im["alpha_opaque"]
    assert (a[:, :4, 3] != 255).any() and (a[:, 4:, 3] == 255).all()
    # exactly one half walks the second pass: a three-subset mode wins one block, the other is coded exactly by the first
    # pass (a zero-error block ends its search there)
    for name, gated, flat in (("gated_flat", 0, 1), ("flat_gated", 1, 0)):
        ref = _ref(name, 2, False)
        assert _mode_numbers(ref)[gated] in (0, 2), name
        dec = O.decode(ref, BC7, 8, 4)
        assert np.array_equal(dec[:, 4*flat:4*flat + 4], im[name][:, 4*flat:4*flat + 4]), name
        assert len(np.unique(im[name][:, 4*flat:4*flat + 4].reshape(-1, 4), axis=0)) == 1


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
