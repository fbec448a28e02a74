"""ETC1 / ETC2 / EAC on the GPU beyond the photo: every colour mode, every EAC table and multiplier, the laws between
what the encoder writes and what a decoder reads, partial workgroups, pitched / bottom-up / device / batched sources
and special values.  The cases and the laws live in tests/etc_cases.py; tests/test_etc_cases.py holds them for the
oracle alone."""
import functools

import numpy as np
import pytest

import etc_cases as C
import oracle_lib as O
from cuttlefish_amd import ColorSpace, Format, Type, make_params, synth

pytestmark = pytest.mark.gpu

COLOUR = [C.ETC1, C.RGB, C.A1, C.A8]
EAC = [(C.R11, C.UNORM), (C.R11, C.SNORM), (C.RG11, C.UNORM), (C.RG11, C.SNORM)]
# all six formats, EAC signed for R11 and unsigned for RG11
SIX = [(C.ETC1, C.UNORM), (C.RGB, C.UNORM), (C.A1, C.UNORM), (C.A8, C.UNORM), (C.R11, C.SNORM), (C.RG11, C.UNORM)]


def _params(fmt, typ=0, quality=2, color_space=0, mask=(1, 1, 1, 1)):
    return make_params(Format(int(fmt)), Type(int(typ)), quality, color_space=ColorSpace(int(color_space)),
                       color_mask=tuple(bool(m) for m in mask))


def _gpu(ctx, img, fmt, typ=0, quality=2, **kw):
    return ctx.encode([img], _params(fmt, typ, quality, **kw))[0]


@functools.lru_cache(maxsize=None)
def _ref_cached(key, fmt, typ, quality, color_space, mask):
    return O.encode(_SOURCES[key](), int(fmt), typ=int(typ), quality=quality, threads=16, color_space=color_space,
                    mask=mask)


def _ref(img, fmt, typ=0, quality=2, color_space=0, mask=(1, 1, 1, 1)):
    return O.encode(img, int(fmt), typ=int(typ), quality=quality, threads=16, color_space=color_space, mask=mask)


_SOURCES = {"colour": C.colour_source, "a1": C.a1_source, "a8": C.a8_source,
            "eac0": lambda: C.eac_source(C.UNORM), "eac1": lambda: C.eac_source(C.SNORM)}


def _source_key(fmt, typ=0):
    return {C.A1: "a1", C.A8: "a8", C.R11: "eac%d" % typ, C.RG11: "eac%d" % typ}.get(int(fmt), "colour")


def _wide(fmt, typ=0):
    fmt = int(fmt)
    if fmt in (C.R11, C.RG11):
        return C.eac_source(typ, wide=True)
    return {C.A1: C.a1_source, C.A8: C.a8_source}.get(fmt, C.colour_source)(wide=True)


def _describe(blocks, fmt, typ):
    """the mode (colour) or (base, multiplier, table) (EAC) of blocks, for a failure message"""
    fmt, bs = int(fmt), C.block_bytes(fmt)
    if fmt in (C.R11, C.RG11):
        return [tuple(int(v[0]) for v in C.eac_fields(b[:8], int(typ) == C.SNORM)) for b in blocks]
    mode, flip = C.mode_of(blocks[:, bs - 8:], fmt == C.A1)
    return ["%s%s" % (C.MODE_NAMES[m], " flip %d" % f if m <= C.DIFFERENTIAL else "") for m, f in zip(mode, flip)]


def _assert_same(ref, got, fmt, typ, what):
    bs = C.block_bytes(fmt)
    assert ref.size == got.size, what
    r, g = ref.reshape(-1, bs), got.reshape(-1, bs)
    bad = np.flatnonzero((r != g).any(axis=1))
    if bad.size:
        print("%s: oracle %s\nGPU    %s" % (what, _describe(r[bad[:10]], fmt, typ), _describe(g[bad[:10]], fmt, typ)))
    assert bad.size == 0, "%s: %d blocks differ, first %s" % (what, bad.size, bad[:10])


def _assert_decoders_agree(ctx, payload, fmt, typ, w, h):
    got, bad = ctx.decode(payload, Format(int(fmt)), Type(int(typ)), w, h)
    assert bad == 0
    if int(fmt) in (C.R11, C.RG11):
        want = O.decode_eac(payload, int(fmt), w, h, int(typ))
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want)
    else:
        assert np.array_equal(got, O.decode_etc(payload, int(fmt), w, h))


# ---- byte parity on the mode sources ------------------------------------------------------------------------

@pytest.mark.parametrize("quality", C.LEVELS)
@pytest.mark.parametrize("fmt", COLOUR)
def test_colour_mode_sources_match_the_oracle(gpu_ctx, fmt, quality):
    key = _source_key(fmt)
    src = _SOURCES[key]()
    ref = _ref_cached(key, fmt, 0, quality, 0, (1, 1, 1, 1))
    for img in (src, C.as_float(src)):
        got = _gpu(gpu_ctx, img, fmt, 0, quality)
        _assert_same(ref, got, fmt, 0, str(img.dtype))
        C.check_mode_counts(got, fmt, quality)
    _assert_decoders_agree(gpu_ctx, got, fmt, 0, src.shape[1], src.shape[0])


@pytest.mark.parametrize("quality", C.LEVELS)
@pytest.mark.parametrize("fmt,typ", EAC)
def test_eac_sources_match_the_oracle(gpu_ctx, fmt, typ, quality):
    key = _source_key(fmt, typ)
    src = _SOURCES[key]()
    ref = _ref_cached(key, fmt, typ, quality, 0, (1, 1, 1, 1))
    got = _gpu(gpu_ctx, src, fmt, typ, quality)
    _assert_same(ref, got, fmt, typ, "float32")
    C.check_eac_counts(got, typ)
    _assert_decoders_agree(gpu_ctx, got, fmt, typ, src.shape[1], src.shape[0])
    # the same image as RGBA8 (the colour source: 256 of the levels) and that as float32 (u8/255)
    img8 = C.colour_source()
    ref8 = _ref(img8, fmt, typ, quality)
    for img in (img8, C.as_float(img8)):
        _assert_same(ref8, _gpu(gpu_ctx, img, fmt, typ, quality), fmt, typ, "colour source as %s" % img.dtype)


@pytest.mark.parametrize("quality", [1, 3])
@pytest.mark.parametrize("fmt", [C.RGB, C.A1, C.A8])
def test_srgb_metric_and_colour_mask(gpu_ctx, fmt, quality):
    key = _source_key(fmt)
    src = _SOURCES[key]()
    for cs, mask in ((1, (1, 1, 1, 1)), (0, (1, 0, 1, 1)), (1, (1, 0, 1, 1))):
        ref = _ref_cached(key, fmt, 0, quality, cs, mask)
        got = _gpu(gpu_ctx, src, fmt, 0, quality, color_space=cs, mask=mask)
        _assert_same(ref, got, fmt, 0, "colour space %d mask %s" % (cs, mask))


# ---- laws, with the GPU as the encoder ------------------------------------------------------------------------

@pytest.mark.parametrize("quality", [0, 2, 4])
def test_flat_laws(gpu_ctx, quality):
    enc = functools.partial(_gpu, gpu_ctx)
    C.check_flat_alpha_law(enc, quality)
    for fmt in COLOUR:
        C.check_flat_colour_law(enc, fmt, quality)
    for fmt, typ in EAC:
        C.check_flat_r11_law(enc, fmt, typ, quality)


@pytest.mark.parametrize("fmt", COLOUR)
def test_no_colour_block_is_worse_than_the_flat_block(gpu_ctx, fmt):
    bad = []
    for name, img in C.bound_sources():
        for q in range(C.BOUND_FROM[fmt], 5):
            n, ratio = C.over_flat_bound_rgb(_gpu(gpu_ctx, img, fmt, 0, q), img, fmt)
            if n:
                bad.append("%s level %d: %d blocks, worst %.2f x the flat block" % (name, q, n, ratio))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("typ", [C.UNORM, C.SNORM])
def test_no_eac_block_is_worse_than_the_flat_block(gpu_ctx, typ):
    photo = C.as_float(synth.photo(128, 64, seed=5))
    for i, src in enumerate([C.eac_source(typ), photo*2 - 1 if typ else photo, C.as_float(C.noise_image())]):
        vals = C.r11_levels(src, typ, 2)
        for q in C.LEVELS:
            assert C.over_flat_bound_eac(_gpu(gpu_ctx, src, C.RG11, typ, q), vals, typ, C.RG11) == (0, 0.0), (i, q)
    a8 = C.a8_source()
    for q in C.LEVELS:
        assert C.over_flat_bound_eac(_gpu(gpu_ctx, a8, C.A8, 0, q), a8[..., 3], 0, C.A8) == (0, 0.0), q


@pytest.mark.parametrize("fmt", COLOUR)
def test_unorm8_boundaries(gpu_ctx, fmt):
    """the float32 -> byte conversion of the loader against numpy on every tie and its neighbours, +-Inf, -0 and NaN
    of both signs; then against the oracle"""
    got = C.check_unorm8_law(functools.partial(_gpu, gpu_ctx), fmt, 1)
    f = C.unorm8_boundary_image()
    _assert_same(_ref(f, fmt, 0, 1), got, fmt, 0, "float32 boundaries")
    _assert_decoders_agree(gpu_ctx, got, fmt, 0, f.shape[1], f.shape[0])


@pytest.mark.parametrize("fmt,typ", EAC)
def test_r11_boundaries(gpu_ctx, fmt, typ):
    """the float32 -> 11-bit conversion against numpy on every tie and its neighbours; then against the oracle, NaN
    included (level 0 on both sides)"""
    got = C.check_r11_law(functools.partial(_gpu, gpu_ctx), fmt, typ, 1)
    f = C.r11_boundary_image(int(typ) == C.SNORM)
    assert np.isnan(f[..., 0]).any()
    _assert_same(_ref(f, fmt, typ, 1), got, fmt, typ, "float32 boundaries")
    _assert_decoders_agree(gpu_ctx, got, fmt, typ, f.shape[1], f.shape[0])


# ---- launches and source paths --------------------------------------------------------------------------------

SHAPES = [(w, h, ragged) for w in (1, 3, 4, 5, 15, 16, 17, 33) for h in (1, 2) for ragged in (False, True)]


def _crops(src):
    crops = [src[:(4*h - 1 if ragged else 4*h), :(4*w - 3 if ragged else 4*w)] for w, h, ragged in SHAPES]
    assert all(c.shape[1] in (4*w, 4*w - 3) and c.shape[0] in (4*h, 4*h - 1) for c, (w, h, _) in zip(crops, SHAPES))
    return crops


@pytest.mark.parametrize("quality", [1, 3])
@pytest.mark.parametrize("fmt,typ,cs", [(f, t, 0) for f, t in SIX] + [(C.A1, C.UNORM, 1)])
def test_partial_workgroups(gpu_ctx, fmt, typ, cs, quality):
    """crops from block column 0: fewer blocks than a workgroup's 16, than a wavefront's 4, one more than either,
    whole and ragged texel sizes; each alone (plain launch) and all in one call (batched launch).  RGB8A1 also
    under the sRGB metric: ragged blocks of that combination once came out wrong."""
    crops = _crops(_wide(fmt, typ))
    refs = [_ref(c, fmt, typ, quality, cs) for c in crops]
    for shape, crop, ref in zip(SHAPES, crops, refs):
        _assert_same(ref, _gpu(gpu_ctx, crop, fmt, typ, quality, color_space=cs), fmt, typ, "crop %s alone" % (shape,))
    together = gpu_ctx.encode(crops, _params(fmt, typ, quality, cs))
    for shape, got, ref in zip(SHAPES, together, refs):
        _assert_same(ref, got, fmt, typ, "crop %s in one call" % (shape,))


@pytest.mark.parametrize("fmt,typ", [(C.A8, C.UNORM), (C.RG11, C.UNORM)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_pitched_and_bottom_up_host_views(gpu_ctx, dtype, fmt, typ):
    src = _wide(fmt, typ)[:45, :131]
    img = src if src.dtype == dtype else (C.as_float(src) if dtype == np.float32 else C.unorm8_levels(src))
    assert img.shape == (45, 131, 4) and img.dtype == dtype
    ref = _ref(img, fmt, typ, 2)
    wide = np.full((45, 140, 4), 7, dtype)
    wide[:, :131] = img
    pitched = wide[:, :131]
    assert pitched.strides[0] > 131*4*img.itemsize
    _assert_same(ref, _gpu(gpu_ctx, pitched, fmt, typ, 2), fmt, typ, "pitched")
    bottom_up = np.ascontiguousarray(img[::-1])[::-1]
    assert bottom_up.strides[0] < 0
    _assert_same(ref, _gpu(gpu_ctx, bottom_up, fmt, typ, 2), fmt, typ, "bottom-up")


@pytest.mark.parametrize("fmt", [C.RGB, C.A8])
@pytest.mark.parametrize("dtype,pixel_type", [(np.uint8, 0), (np.float32, 1)])
def test_device_buffers_pixel_aligned_with_padded_pitch(gpu_ctx, dtype, pixel_type, fmt):
    """encode_device: base advanced by one pixel (4-byte aligned for RGBA8, 16-byte for RGBA32F), pitch padded by 3
    pixels; the output buffer is 32 bytes longer than the payload and its tail stays as it was."""
    torch = pytest.importorskip("torch")
    src = _wide(fmt)[:45, :131]
    img = src if dtype == np.uint8 else C.as_float(src)
    h, w = img.shape[:2]
    ref = _ref(img, fmt, 0, 2)
    pitch_px = w + 3
    host = np.full((1 + h*pitch_px, 4), 3, dtype)                             # one pixel in front of the surface
    host[1:].reshape(h, pitch_px, 4)[:, :w] = img
    psize = 4*img.itemsize
    dsrc = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).cuda()
    dout = torch.full((ref.size + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_ctx.encode_device([dict(pixels=dsrc.data_ptr() + psize, pixel_type=pixel_type, width=w, height=h,
                                row_pitch_bytes=pitch_px*psize, out=dout.data_ptr(), out_capacity=ref.size)],
                          _params(fmt, 0, 2))
    torch.cuda.synchronize()
    out = dout.cpu().numpy()
    _assert_same(ref, out[:ref.size], fmt, 0, "device path")
    assert (out[ref.size:] == 0xAB).all()


@pytest.mark.parametrize("fmt,typ", [(C.A8, C.UNORM), (C.RG11, C.UNORM)])
def test_mip_chain_in_one_call_is_one_batched_launch(gpu_ctx, fmt, typ):
    src = _SOURCES[_source_key(fmt, typ)]()
    chain = [np.ascontiguousarray(src[:n, :n]) for n in (64, 32, 16, 8, 4, 2, 1)]
    alone = [_gpu(gpu_ctx, c, fmt, typ, 2) for c in chain]
    gpu_ctx.profile_begin()
    together = gpu_ctx.encode(chain, _params(fmt, typ, 2))
    _, launches = gpu_ctx.profile_end()
    assert 1 <= launches < len(chain)
    for c, a, t in zip(chain, alone, together):
        _assert_same(a, t, fmt, typ, "%d x %d alone vs in the chain" % c.shape[:2])
        _assert_same(_ref(c, fmt, typ, 2), t, fmt, typ, "%d x %d" % c.shape[:2])


@pytest.mark.parametrize("fmt,typ", SIX)
def test_special_values(gpu_ctx, fmt, typ):
    """+-NaN, +-Inf, -0, -1, 1e9 and 6e-8 over 2 % of all four channels of a float32 photo"""
    f = C.sprinkle_specials(synth.photo(68, 44, seed=12))
    nan = np.isnan(f)
    assert nan[..., 0].any() and nan[..., 3].any() and np.signbit(f[nan]).any() and not np.signbit(f[nan]).all()
    _assert_same(_ref(f, fmt, typ, 2), _gpu(gpu_ctx, f, fmt, typ, 2), fmt, typ, "specials")
