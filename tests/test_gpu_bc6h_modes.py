"""BC6H on the GPU beyond the probe images: every mode's bit runs, the laws between what the encoder writes and
what a decoder reads, partial workgroups, pitched / bottom-up / device / batched sources and special values.
The cases and the laws live in tests/bc6h_cases.py; tests/test_bc6h_cases.py holds them for the oracle alone."""
import functools

import numpy as np
import pytest

import bc6h_cases as C
import oracle_lib as O
from cuttlefish_amd import Format, Type, make_params, synth

pytestmark = pytest.mark.gpu
BC6H = int(Format.BC6H)
TYPES = [Type.UFloat, Type.Float]


def _gpu(ctx, img, typ, quality):
    return ctx.encode([img], make_params(Format.BC6H, Type(int(typ)), quality))[0]


def _ref(img, typ, quality):
    return O.encode(img, BC6H, typ=int(typ), quality=quality, threads=16)


@functools.lru_cache(maxsize=None)
def _source(typ):
    src = C.mode_complete_source(int(typ))
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def _wide_source(typ):
    """the same construction 36 x 12 blocks large: room for crops 33 blocks wide"""
    src = C.mode_complete_source(int(typ), seed=2025, bx=36, by=12)
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def _source_ref(typ, quality):
    return _ref(_source(typ), typ, quality)


def _assert_same(ref, got, what):
    r, g = ref.reshape(-1, 16), got.reshape(-1, 16)
    bad = np.flatnonzero((r != g).any(axis=1))
    assert bad.size == 0, "%s: %d blocks differ, first %s; oracle modes %s, GPU modes %s" % (
        what, bad.size, bad[:10], C.mode_of(r[bad[:10]]), C.mode_of(g[bad[:10]]))


def _assert_decoders_agree(ctx, payload, w, h, typ):
    got, bad = ctx.decode(payload, Format.BC6H, Type(int(typ)), w, h)
    assert bad == 0
    want = O.decode_bc6h(payload, w, h, int(typ))
    assert np.array_equal(C.half_bits(got), C.half_bits(want))


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("quality", C.LEVELS)
def test_mode_complete_source_matches_the_oracle(gpu_ctx, typ, quality):
    src = _source(typ)
    ref = _source_ref(typ, quality)
    for img in (src, src.astype(np.float32)):
        got = _gpu(gpu_ctx, img, typ, quality)
        _assert_same(ref, got, str(img.dtype))
        C.check_mode_counts(got, quality)
    _assert_decoders_agree(gpu_ctx, got, src.shape[1], src.shape[0], typ)


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("quality", [0, 2, 4])
def test_flat_law(gpu_ctx, typ, quality):
    C.check_flat_law(lambda img, t, q: _gpu(gpu_ctx, img, t, q), int(typ), quality)


@pytest.mark.parametrize("typ", TYPES)
def test_byte_law(gpu_ctx, typ):
    enc = lambda img, t, q: _gpu(gpu_ctx, img, t, q)       # noqa: E731
    for q in (0, 2):
        C.check_byte_law(enc, int(typ), q)
        img8 = C.bytes_flat()
        _assert_same(_ref(img8, typ, q), enc(img8, typ, q), "bytes")


@pytest.mark.parametrize("typ", TYPES)
def test_float32_law(gpu_ctx, typ):
    """v_cvt_f16_f32 against numpy's RNE on every boundary, NaN of both signs included (two GPU encodes), then
    against the oracle's packHardwareHalfFloat."""
    got = C.check_float32_law(lambda img, t, q: _gpu(gpu_ctx, img, t, q), int(typ), 1)
    f = C.half_boundaries(int(typ) == C.FLOAT)
    _assert_same(_ref(f, typ, 1), got, "float32 boundaries")
    _assert_decoders_agree(gpu_ctx, got, f.shape[1], f.shape[0], typ)


@pytest.mark.parametrize("typ", TYPES)
def test_no_block_is_worse_than_the_flat_block(gpu_ctx, typ):
    bad = []
    for name, img in C.bound_sources(int(typ)):
        for q in C.LEVELS:
            got = _gpu(gpu_ctx, img, typ, q)
            n, ratio = C.over_flat_bound(got, img, int(typ))
            if n:
                bad.append("%s level %d: %d blocks, worst %.1f x the flat block" % (name, q, n, ratio))
        _assert_decoders_agree(gpu_ctx, got, img.shape[1], img.shape[0], typ)
    assert not bad, "\n".join(bad)


SHAPES = [(w, h, ragged) for w in (1, 3, 4, 5, 15, 16, 17, 33) for h in (1, 2) for ragged in (False, True)]


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("quality", [1, 3])
def test_partial_workgroups(gpu_ctx, typ, quality):
    """crops from block column 0 (every mode within 14 columns): fewer blocks than a workgroup's 16, than a
    wavefront's 4, one more than either, an odd count for the two-blocks-per-pass pairing, whole and ragged
    texel sizes; each alone (plain launch) and all in one call (batched launch)."""
    src = _wide_source(typ)
    crops = [src[:(4*h - 1 if ragged else 4*h), :(4*w - 3 if ragged else 4*w)] for w, h, ragged in SHAPES]
    assert all(c.shape[1] in (4*w, 4*w - 3) and c.shape[0] in (4*h, 4*h - 1) for c, (w, h, _) in zip(crops, SHAPES))
    refs = [_ref(c, typ, quality) for c in crops]
    for shape, crop, ref in zip(SHAPES, crops, refs):
        _assert_same(ref, _gpu(gpu_ctx, crop, typ, quality), "crop %s alone" % (shape,))
    together = gpu_ctx.encode(crops, make_params(Format.BC6H, typ, quality))
    for shape, got, ref in zip(SHAPES, together, refs):
        _assert_same(ref, got, "crop %s in one call" % (shape,))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_pitched_and_bottom_up_host_views(gpu_ctx, dtype):
    typ, q = Type.Float, 2
    img = _wide_source(typ)[:45, :131].astype(dtype)
    assert img.shape == (45, 131, 4)
    ref = _ref(img, typ, q)
    wide = np.full((45, 140, 4), 7, dtype)
    wide[:, :131] = img
    pitched = wide[:, :131]
    assert pitched.strides[0] > 131*4*img.itemsize
    _assert_same(ref, _gpu(gpu_ctx, pitched, typ, q), "pitched")
    bottom_up = np.ascontiguousarray(img[::-1])[::-1]
    assert bottom_up.strides[0] < 0
    _assert_same(ref, _gpu(gpu_ctx, bottom_up, typ, q), "bottom-up")


@pytest.mark.parametrize("dtype,pixel_type", [(np.float16, 2), (np.float32, 1)])
def test_device_buffers_pixel_aligned_with_padded_pitch(gpu_ctx, dtype, pixel_type):
    """encode_device: base advanced by one pixel (8-byte aligned for halves, not 16), pitch padded by 3 pixels;
    the output buffer is 32 bytes longer than the payload and its tail stays as it was."""
    torch = pytest.importorskip("torch")
    typ, q = Type.UFloat, 2
    img = _wide_source(typ)[:45, :131].astype(dtype)
    h, w = img.shape[:2]
    ref = _ref(img, typ, q)
    pitch_px = w + 3
    host = np.full((1 + h*pitch_px, 4), 3, dtype)                             # one pixel in front of the surface
    host[1:].reshape(h, pitch_px, 4)[:, :w] = img
    psize = 4*img.itemsize
    dsrc = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).cuda()
    dout = torch.full((ref.size + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_ctx.encode_device([dict(pixels=dsrc.data_ptr() + psize, pixel_type=pixel_type, width=w, height=h,
                                row_pitch_bytes=pitch_px*psize, out=dout.data_ptr(), out_capacity=ref.size)],
                          make_params(Format.BC6H, typ, q))
    torch.cuda.synchronize()
    out = dout.cpu().numpy()
    _assert_same(ref, out[:ref.size], "device path")
    assert (out[ref.size:] == 0xAB).all()


def test_mip_chain_in_one_call_is_one_batched_launch(gpu_ctx):
    typ, q = Type.UFloat, 2
    src = _source(typ)
    chain = [np.ascontiguousarray(src[:n, :n]) for n in (64, 32, 16, 8, 4, 2, 1)]
    params = make_params(Format.BC6H, typ, q)
    alone = [_gpu(gpu_ctx, c, typ, q) for c in chain]
    gpu_ctx.profile_begin()
    together = gpu_ctx.encode(chain, params)
    _, launches = gpu_ctx.profile_end()
    assert 1 <= launches < len(chain)
    for c, a, t in zip(chain, alone, together):
        _assert_same(a, t, "%d x %d alone vs in the chain" % c.shape[:2])
        _assert_same(_ref(c, typ, q), t, "%d x %d" % c.shape[:2])


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("quality", [1, 2])
def test_special_values(gpu_ctx, typ, quality):
    """+-NaN, +-Inf, -0, -1, +-1e9, 6e-8 and 65504 over 2 % of the probe's RGB, as RGBA32F and (rounded by numpy)
    RGBA16F; the RGBA8 source has no such values and stays plain."""
    f = C.sprinkle_specials(synth.hdr_probe(68, 44, seed=12, signed=typ == Type.Float))
    assert np.isnan(f).any() and np.signbit(f[np.isnan(f)]).any() and not np.signbit(f[np.isnan(f)]).all()
    for img in (f, C.to_half(f), synth.photo(68, 44, seed=12)):
        _assert_same(_ref(img, typ, quality), _gpu(gpu_ctx, img, typ, quality), str(img.dtype))
