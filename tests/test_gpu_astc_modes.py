"""ASTC on the GPU where byte parity means something: sources on which four and three partitions, the luminance and
base + scale endpoint modes, void extents and every weight range actually win (tests/astc_cases.py; the census
conditions of tests/test_astc_cases.py hold for the kernel's payload too), the metric flags on multi-partition content,
float forms of the sources, the HDR profiles on painted content, and every launch shape of the kernel's plan at a
row's ragged end -- alone, batched and from a pitched bottom-up device surface."""
import functools

import numpy as np
import pytest

import astc_cases as C
import oracle_lib as O
from cuttlefish_amd import Alpha, ColorSpace, Format, Type, make_params

pytestmark = pytest.mark.gpu


def _name(fmt):
    return "%dx%d" % C.FOOT[fmt]


def _params(fmt, quality, typ=0, alpha=1, color_space=0, mask=(1, 1, 1, 1)):
    return make_params(Format(int(fmt)), Type(int(typ)), quality, alpha=Alpha(int(alpha)),
                       color_space=ColorSpace(int(color_space)), color_mask=tuple(bool(m) for m in mask))


def _gpu(ctx, img, fmt, quality, **kw):
    return ctx.encode([img], _params(fmt, quality, **kw))[0]


def _assert_same(ref, got, fmt, what):
    assert ref.size == got.size, what
    r, g = ref.reshape(-1, 16), np.asarray(got).reshape(-1, 16)
    bad = np.flatnonzero((r != g).any(axis=1))
    if bad.size:
        print(what)
        for i, a, b in zip(bad[:6], C.describe(r[bad[:6]], fmt), C.describe(g[bad[:6]], fmt)):
            print("block %d\n  oracle %s\n  GPU    %s" % (i, a, b))
    assert bad.size == 0, "%s: %d blocks differ, first %s" % (what, bad.size, bad[:10])


def _assert_decoders_agree(ctx, payload, fmt, w, h):
    got, bad = ctx.decode(payload, Format(int(fmt)), Type.UNorm, w, h)
    want, want_bad = O.decode_astc(payload, int(fmt), w, h)
    assert bad == want_bad == 0
    assert np.array_equal(got, want)


# ---- byte parity and census on the sources ---------------------------------------------------------------------

GROUPS = [(fmt, name, keys) for name, keys in (("four", C.PAINTED4), ("three", C.PAINTED3)) for fmt in C.FORMATS] + \
         [(fmt, "plain", C.PLAIN) for fmt in C.FIVE]


@pytest.mark.parametrize("fmt,keys", [g[::2] for g in GROUPS], ids=["%s-%s" % (_name(g[0]), g[1]) for g in GROUPS])
def test_sources_match_the_oracle(gpu_ctx, fmt, keys):
    """painted with four partitions at Highest, with three at Normal, High and Highest (all 14 footprints); grey,
    scaled, void extent and ramps at all five levels (five footprints): the oracle's bytes, the census conditions on
    the kernel's own payload, and the GPU decoder on it"""
    for key in keys:
        img = C.source(key, fmt)
        for q in C.levels_of(key):
            got = _gpu(gpu_ctx, img, fmt, q)
            _assert_same(C.ref(key, fmt, q), got, fmt, "%s %s level %d" % (key, _name(fmt), q))
            C.check_census(key, fmt, q, got)
            _assert_decoders_agree(gpu_ctx, got, fmt, img.shape[1], img.shape[0])


METRICS = [dict(color_space=1), dict(color_space=1, alpha=0), dict(alpha=2), dict(alpha=0), dict(mask=(1, 0, 1, 1)),
           dict(alpha=3, color_space=1, mask=(0, 1, 1, 1))]


@pytest.mark.parametrize("parts", [3, 4])
@pytest.mark.parametrize("fmt", C.METRIC_FORMATS, ids=_name)
def test_metric_flags_on_multi_partition_content(gpu_ctx, fmt, parts):
    """sRGB (the perceptual channel weights), the alpha weight on and off and a colour mask enter the per-subset error
    of the multi-partition path"""
    for kind in C.KINDS:
        key = ("painted", parts, kind)
        img = C.source(key, fmt)
        for q in C.levels_of(key):
            if q == C.HIGH:
                continue
            for kw in METRICS:
                ref = C.ref(key, fmt, q, **kw)
                _assert_same(ref, _gpu(gpu_ctx, img, fmt, q, **kw), fmt, "%s %s level %d %s" % (key, _name(fmt), q, kw))


@pytest.mark.parametrize("fmt", C.FIVE, ids=_name)
def test_float_forms_of_the_sources(gpu_ctx, fmt):
    """RGBA32F and RGBA16F sources are quantised to UNORM8 at the loader ("Float sources on the
    ASTC-LDR and ETC legs"), so u8 / 255 as float32 or float16 gives the bytes of the RGBA8 encode everywhere, void
    extents included; the float void-extent source, whose values are not on the byte grid, gives the oracle's bytes
    for that float source"""
    for key in (("grey", True), ("painted", 4, "grey"), ("painted", 3, "alpha"), ("void", "u8")):
        img = C.source(key, fmt)
        q = C.HIGHEST if key[0] == "painted" else C.NORMAL
        for dtype in (np.float32, np.float16):
            f = C.as_float(img, dtype)
            assert np.array_equal(C.unorm8(f), img)
            _assert_same(C.ref(key, fmt, q), _gpu(gpu_ctx, f, fmt, q), fmt, "%s as %s" % (key, np.dtype(dtype).name))
    f = C.source(("void", "f32"), fmt)
    half = np.ascontiguousarray(f.astype(np.float16))
    for q in (0, C.NORMAL):
        _assert_same(C.ref(("void", "f32"), fmt, q), _gpu(gpu_ctx, f, fmt, q), fmt, "float void extent level %d" % q)
        _assert_same(O.encode(half, fmt, quality=q), _gpu(gpu_ctx, half, fmt, q), fmt, "half void extent level %d" % q)


# ---- HDR profiles ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [2, 3, 4])
@pytest.mark.parametrize("fmt", C.HDR_FORMATS, ids=_name)
def test_hdr_painted_sources_match_the_oracle(gpu_ctx, fmt, parts):
    """the painted sources at exposures 2^-4 .. 2^8 under both alpha profiles, all levels; what the oracle reaches
    on them is in tests/test_astc_cases.py::test_hdr_census_of_the_oracle"""
    for alpha, mode in C.HDR_ALPHAS.items():
        key = ("hdr_painted", parts, alpha)
        img = C.source(key, fmt)
        for q in range(5):
            ref = C.ref(key, fmt, q, typ=C.UFLOAT, alpha=mode)
            got = _gpu(gpu_ctx, img, fmt, q, typ=C.UFLOAT, alpha=mode)
            _assert_same(ref, got, fmt, "%s %s level %d" % (key, _name(fmt), q))


# ---- launch shapes ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sweep_crops(fmt, quality, hdr):
    """three block rows, the last one a texel short; every width of the sweep as a crop from block column 0 that
    ends half a block into its last block"""
    bw, bh = C.FOOT[fmt]
    wide = C.sweep_image(bw, bh, hdr)
    return [np.ascontiguousarray(wide[:, :bx*bw - bw//2]) for bx in C.SWEEP[(fmt, quality, hdr)][1]]


@pytest.mark.parametrize("hdr", [False, True], ids=["ldr", "hdr"])
@pytest.mark.parametrize("quality", C.SHAPE_LEVELS)
@pytest.mark.parametrize("fmt", C.SHAPE_FORMATS, ids=_name)
def test_every_launch_shape_at_a_ragged_row_end(gpu_ctx, fmt, quality, hdr):
    """tests/test_astc_cases.py::test_launch_sweep_reaches_every_shape_of_the_plan names the shapes these widths
    select.  Each width alone (the plain grid), then all in one call (the batched grid over the workgroups of all
    surfaces)."""
    typ = C.UFLOAT if hdr else 0
    widths = C.SWEEP[(fmt, quality, hdr)][1]
    crops = _sweep_crops(fmt, quality, hdr)
    refs = [O.encode(c, fmt, typ=typ, quality=quality, threads=16) for c in crops]
    for bx, crop, ref in zip(widths, crops, refs):
        assert ref.size == bx*3*16
        _assert_same(ref, _gpu(gpu_ctx, crop, fmt, quality, typ=typ), fmt, "%d blocks per row alone" % bx)
    together = gpu_ctx.encode(crops, _params(fmt, quality, typ=typ))
    for bx, got, ref in zip(widths, together, refs):
        _assert_same(ref, got, fmt, "%d blocks per row in one call" % bx)


@pytest.mark.parametrize("fmt,quality", [(47, C.NORMAL), (56, C.HIGH)], ids=["6x6-2", "12x12-3"])
def test_pitched_bottom_up_device_surface(gpu_ctx, fmt, quality):
    """encode_device from a surface whose rows lie bottom-up in device memory, three pixels of padding per row; the
    output buffer is 32 bytes longer than the payload and its tail stays as it was"""
    torch = pytest.importorskip("torch")
    img = _sweep_crops(fmt, quality, False)[-1]
    h, w = img.shape[:2]
    ref = O.encode(img, fmt, quality=quality, threads=16)
    pitch = (w + 3)*4
    host = np.full((h, w + 3, 4), 9, np.uint8)
    host[::-1, :w] = img                                            # memory row 0 is the image's last row
    dsrc = torch.from_numpy(host.reshape(-1).copy()).cuda()
    dout = torch.full((ref.size + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_ctx.encode_device([dict(pixels=dsrc.data_ptr() + (h - 1)*pitch, pixel_type=0, width=w, height=h,
                                row_pitch_bytes=-pitch, out=dout.data_ptr(), out_capacity=ref.size)],
                          _params(fmt, quality))
    torch.cuda.synchronize()
    out = dout.cpu().numpy()
    _assert_same(ref, out[:ref.size], fmt, "bottom-up device surface")
    assert (out[ref.size:] == 0xAB).all()
