"""GPU parity of BC7 with the palette of the selector search built from a line and a row of weight bytes
(csrc/bc7_packed.h: pal_line / pal_at, cf_bc7_make_weights; csrc/bc7_encode.hip: assign_lsq_lane): every payload must
equal the CPU oracle's byte for byte, at levels 0..4, with both metrics and both pixel types.

The launches are the smallest that reach each path of the kernel: 4x4 (one block, no pair), 8x4 (one pair), 12x4 (a pair
and a single in one wave) and 20x4 (two waves).  Their blocks come from seeded generators; which mode each turns out
to be is asserted below, on the oracle's output alone:
  flat      one colour (the axis has length 0: no reciprocal is taken, every palette entry is the same colour)
  twocol    two colours (the least-squares system of the refit is singular; at Normal modes 3 and 5 in every rotation)
  onech     one channel varies, the others are constant
  aramp     a colour line with an alpha ramp of its own (mode 4, rotation 0)
  rotramp   a colour channel varies on its own, the others and alpha follow one line (mode 4, rotations 1..3)
  two7      two colours with their own alpha laid out by a two-subset partition (modes 7 and 5)
  noise     seeded noise, with and without alpha
  grad      planar colour gradients (at Normal modes 0, 1, 2, 3)
  two2      two gradients laid out by a two-subset partition (modes 1 and 3)
  grad3     three gradients laid out by a three-subset partition (modes 0 and 2)
  alpha4    a colour line with random alpha (modes 4 and 6)
The seeds were chosen on the CPU so that at Normal every mode wins a block: modes 1, 3, 5, 6 and 7 in the first pass,
modes 0, 2 and 4, which Normal reaches in its second pass alone, there.  Index widths 2, 3 and 4 (mode 6's two
palette halves) all occur among the winners, so every row of the weight table is read by a fit that wins."""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params
from test_bc7_cand_words import PART2, PART3

BC7 = int(Format.BC7)


def flat(seed):
    r = np.random.default_rng(seed)
    b = np.empty((4, 4, 4), np.uint8)
    b[:] = r.integers(0, 256, 4)
    b[..., 3] = 255 if seed % 2 else b[0, 0, 3]
    return b


def twocol(seed):
    r = np.random.default_rng(100 + seed)
    c = r.integers(0, 256, (2, 4))
    c[:, 3] = 255
    lab = r.integers(0, 2, (4, 4))
    lab[0, 0] = 0
    lab[3, 3] = 1
    return c[lab].astype(np.uint8)


def onech(seed):
    r = np.random.default_rng(200 + seed)
    b = np.empty((4, 4, 4), np.uint8)
    b[:] = r.integers(0, 256, 4)
    b[..., 3] = 255
    b[..., seed % 3] = r.integers(0, 256, (4, 4))
    return b


def aramp(seed):
    r = np.random.default_rng(300 + seed)
    c0, c1 = r.integers(0, 256, 3), r.integers(0, 256, 3)
    t = r.random((4, 4, 1))
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(np.rint(c0 + (c1 - c0)*t), 0, 255)
    b[..., 3] = np.clip(np.linspace(r.integers(0, 100), r.integers(120, 256), 16).reshape(4, 4), 0, 255)
    return b


def rotramp(seed):
    r = np.random.default_rng(400 + seed)
    c0, c1 = r.integers(0, 256, 4), r.integers(0, 256, 4)
    t = r.random((4, 4, 1))
    b = np.clip(np.rint(c0 + (c1 - c0)*t), 0, 255).astype(np.uint8)
    b[..., seed % 3] = r.integers(0, 256, (4, 4))
    return b


def two7(seed):
    r = np.random.default_rng(1000 + seed)
    p = PART2[int(r.integers(0, 64))]
    lab = np.array([(p >> t) & 1 for t in range(16)]).reshape(4, 4)
    cols = r.integers(0, 256, (2, 4))
    cols[:, 3] = r.integers(0, 240, 2)
    return np.clip(cols[lab] + r.integers(-3, 4, (4, 4, 4)), 0, 255).astype(np.uint8)


def noise(seed):
    r = np.random.default_rng(500 + seed)
    b = r.integers(0, 256, (4, 4, 4)).astype(np.uint8)
    if seed % 2:
        b[..., 3] = 255
    return b


def grad(seed):
    r = np.random.default_rng(600 + seed)
    yy, xx = np.mgrid[0:4, 0:4]
    b = np.empty((4, 4, 4), np.uint8)
    for c in range(3):
        b[..., c] = np.clip(r.integers(0, 200) + xx*r.integers(-20, 21) + yy*r.integers(-20, 21) + r.integers(-2, 3, (4, 4)), 0, 255)
    b[..., 3] = 255
    return b


def _lines(r, lab, n, spread):
    c0 = r.integers(0, 256, (n, 3))
    c1 = np.clip(c0 + r.integers(-spread, spread + 1, (n, 3)), 0, 255)
    t = r.random((4, 4, 1))
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(np.rint(c0[lab] + (c1[lab] - c0[lab])*t), 0, 255)
    b[..., 3] = 255
    return b


def two2(seed):
    r = np.random.default_rng(700 + seed)
    p = PART2[int(r.integers(0, 64))]
    return _lines(r, np.array([(p >> t) & 1 for t in range(16)]).reshape(4, 4), 2, 50)


def grad3(seed):
    r = np.random.default_rng(2000 + seed)
    p = PART3[int(r.integers(0, 16))]
    return _lines(r, np.array([(p >> (2*t)) & 3 for t in range(16)]).reshape(4, 4), 3, 60)


def alpha4(seed):
    r = np.random.default_rng(seed)
    c0, c1 = r.integers(0, 256, 3), r.integers(0, 256, 3)
    t = r.random((4, 4, 1))
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(c0 + (c1 - c0)*t + r.integers(-3, 4, (4, 4, 3)), 0, 255)
    b[..., 3] = r.integers(0, 255, (4, 4))
    return b


# one row of blocks per launch: 1, 2, 3 and 5 blocks
LAUNCHES = (
    [(flat, 0)], [(flat, 4)], [(twocol, 1)], [(onech, 0)], [(aramp, 0)], [(two7, 1)], [(noise, 1)], [(grad, 1)],
    [(two2, 0), (twocol, 6)], [(rotramp, 0), (grad3, 7)], [(noise, 0), (flat, 1)], [(grad, 3), (two7, 0)],
    [(twocol, 7), (aramp, 1), (grad, 6)], [(two7, 3), (twocol, 2), (noise, 6)], [(grad3, 0), (onech, 1), (alpha4, 0)],
    [(flat, 2), (two2, 11), (rotramp, 1), (grad, 0), (two7, 4)],
    [(rotramp, 2), (noise, 3), (twocol, 4), (onech, 2), (grad, 11)],
    [(noise, 8), (grad3, 10), (flat, 9), (two2, 1), (alpha4, 7)],
)
CASES = [(q, srgb) for srgb in (False, True) for q in range(5)]


@functools.lru_cache(maxsize=None)
def _images(ptype):
    out = []
    for row in LAUNCHES:
        img = np.ascontiguousarray(np.concatenate([g(s) for g, s in row], axis=1))
        if ptype == "f32":
            img = (img.astype(np.float64)/255.0).astype(np.float32)
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _refs(ptype, quality, srgb):
    """The oracle's payloads of one case: computed once, shared, read-only"""
    out = []
    for img in _images(ptype):
        ref = O.encode(img, BC7, quality=quality, threads=1, color_space=1 if srgb else 0)
        ref.setflags(write=False)
        out.append(ref)
    return tuple(out)


def _winners(payload):
    """(mode, rotation) of every block: the mode is the position of the lowest set bit; modes 4 and 5 carry a rotation"""
    out = []
    for blk in payload.reshape(-1, 16):
        v = int(blk[0]) | (int(blk[1]) << 8)
        mode = ((v | 256) & -(v | 256)).bit_length() - 1
        out.append((mode, (v >> (mode + 1)) & 3 if mode in (4, 5) else 0))
    return out


# ---- what the launches are: conditions on the images and on the oracle's output alone (no GPU) ----

def test_launch_shapes():
    shapes = collections.Counter(img.shape[:2] for img in _images("u8"))
    assert set(shapes) == {(4, 4), (4, 8), (4, 12), (4, 20)}
    flat0 = _images("u8")[0]
    assert (flat0 == flat0[0, 0]).all()
    two = _images("u8")[2].reshape(-1, 4)
    assert len({tuple(t) for t in two.tolist()}) == 2


@pytest.mark.parametrize("srgb", [False, True])
def test_every_mode_wins_at_normal(srgb):
    """Modes 1, 3, 5, 6, 7 belong to Normal's first pass; modes 0, 2 and 4 are fitted by its second pass alone"""
    won = [w for ref in _refs("u8", 2, srgb) for w in _winners(ref)]
    modes = collections.Counter(m for m, _ in won)
    for mode in range(8):
        assert modes[mode] >= 1, (mode, sorted(modes.items()))
    if not srgb:
        # every rotation of the two-plane modes (the perceptual metric uses rotation 0 alone)
        assert {r for m, r in won if m == 5} == {0, 1, 2, 3}
        assert {r for m, r in won if m == 4} == {0, 1, 2, 3}


# ---- parity ----

@pytest.mark.gpu
@pytest.mark.parametrize("ptype", ["u8", "f32"])
@pytest.mark.parametrize("quality,srgb", CASES)
def test_payload_equals_oracle(gpu_ctx, ptype, quality, srgb):
    imgs, refs = _images(ptype), _refs(ptype, quality, srgb)
    kw = {"color_space": ColorSpace.sRGB} if srgb else {}
    params = make_params(Format.BC7, Type.UNorm, quality, **kw)
    for i, (img, ref) in enumerate(zip(imgs, refs)):
        got = gpu_ctx.encode([img], params)[0]      # a call of its own: surfaces of one call share a launch
        assert got.size == ref.size == (img.shape[1]//4)*16
        bad = np.flatnonzero((ref.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1))
        assert bad.size == 0, "launch %d (%s): blocks %s differ" % (i, [g.__name__ + str(s) for g, s in LAUNCHES[i]], bad)
