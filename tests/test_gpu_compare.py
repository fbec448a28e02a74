"""GPU quality metrics (csrc/compare.hip) against the numpy restatement (tests/compare_ref.py) applied to the GPU
decoder's output, against the exact integer sums of decode_sse, and through Texture.compare."""
import ctypes

import numpy as np
import pytest

import compare_ref as R
from cuttlefish_amd import CubeFace, Dimension, Format, Texture, Type, api, make_params, synth

pytestmark = pytest.mark.gpu

# one or more pairs of each layout family
RGBA8 = [(29, 0), (36, 0), (40, 0), (47, 0)]
R8RG8 = [(33, 0), (33, 1), (34, 0), (34, 1)]
EAC = [(41, 0), (41, 1), (42, 0), (42, 1)]
HDR = [(35, 4), (35, 5), (47, 4)]
PAIRS = RGBA8 + R8RG8 + EAC + HDR
SIZES = [(64, 64), (37, 61)]          # (w, h): a photo tile and a ragged surface


def _source(fmt, typ, w, h, seed=3):
    """(what the encoder takes, the reference the metrics read)"""
    if typ in (4, 5):
        img = synth.hdr_probe(w, h, seed=seed, signed=typ == 5)
        return img, img
    img = synth.photo(w, h, seed=seed)
    if typ == 1:
        f = (img.astype(np.float32) / 255.0) * 2.0 - 1.0
        return f, f
    return img, img


def _encode(ctx, fmt, typ, src):
    return ctx.encode([src], make_params(fmt, typ, 0))[0]


def _check_against_restatement(got, want, block_map=True):
    for c in range(4):
        if (want["channels"] >> c) & 1:
            assert got.sse[c] == pytest.approx(want["sse"][c], rel=1e-10, abs=1e-300), ("sse", c)
            assert got.ref_max[c] == want["ref_max"][c]
            if np.isnan(want["log_sse"][c]):
                assert np.isnan(got.log_sse[c])
            else:
                assert got.log_sse[c] == pytest.approx(want["log_sse"][c], rel=1e-10, abs=1e-300), ("log", c)
            if np.isnan(want["ssim"][c]):
                assert np.isnan(got.ssim[c])
            else:
                assert abs(got.ssim[c] - want["ssim"][c]) < 1e-5, ("ssim", c, got.ssim[c], want["ssim"][c])
        else:
            assert got.sse[c] == 0.0 and got.ref_max[c] == 0.0 and np.isnan(got.ssim[c])
    assert got.channels == want["channels"]
    assert got.ssim_windows == want["windows"]
    if block_map:
        np.testing.assert_allclose(got.block_errors, want["block_errors"], rtol=1e-6, atol=1e-30)


def _bits(r):
    return (r.texels, r.error_blocks, r.channels, r.ssim_windows,
            np.array(r.sse + r.log_sse + r.ssim + r.ref_max).tobytes(),
            None if r.block_errors is None else r.block_errors.tobytes())


def _device_compare(ctx, payload, ref, fmt, typ, mask=None, ssim=True):
    torch = pytest.importorskip("torch")
    h, w = ref.shape[:2]
    bw, bh, _ = api.query(fmt, typ)
    nb = ((h + bh - 1) // bh) * ((w + bw - 1) // bw)
    d_blk = torch.from_numpy(np.ascontiguousarray(payload)).cuda()
    d_ref = torch.from_numpy(np.ascontiguousarray(ref).view(np.uint8).reshape(-1)).cuda()
    d_res = torch.zeros(ctypes.sizeof(api.CompareResult), dtype=torch.uint8, device="cuda")
    d_map = torch.zeros(nb, dtype=torch.float32, device="cuda")
    pix = {np.uint8: 0, np.float32: 1, np.float16: 2}[ref.dtype.type]
    torch.cuda.synchronize()
    ctx.compare_device(d_blk.data_ptr(), fmt, typ, w, h, d_ref.data_ptr(), pix, ref.strides[0], d_res.data_ptr(),
                       mask=mask, ssim=ssim, block_errors=d_map.data_ptr(), block_errors_capacity=nb)
    res = api.CompareResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    layout, _ = api.decoded_layout(fmt, typ)
    return api.Comparison(res, layout, d_map.cpu().numpy().reshape((h + bh - 1) // bh, (w + bw - 1) // bw))


@pytest.mark.parametrize("size", SIZES, ids=["tile", "ragged"])
@pytest.mark.parametrize("fmt,typ", PAIRS)
def test_compare_matches_restatement(gpu_ctx, fmt, typ, size):
    w, h = size
    src, ref = _source(fmt, typ, w, h)
    payload = _encode(gpu_ctx, fmt, typ, src)
    dec, bad = gpu_ctx.decode(payload, fmt, typ, w, h)
    layout, _ = api.decoded_layout(fmt, typ)
    bw, bh, _ = api.query(fmt, typ)
    want = R.compare(dec, layout, ref, (bw, bh), ssim=True)
    got = gpu_ctx.compare(payload, ref, fmt, typ, ssim=True, block_map=True)
    assert got.texels == w * h and got.error_blocks == bad
    assert got.block_errors.shape == ((h + bh - 1) // bh, (w + bw - 1) // bw)
    _check_against_restatement(got, want)
    # bit-identical on a second call, and through the device path
    assert _bits(gpu_ctx.compare(payload, ref, fmt, typ, ssim=True, block_map=True)) == _bits(got)
    assert _bits(_device_compare(gpu_ctx, payload, ref, fmt, typ)) == _bits(got)


@pytest.mark.parametrize("fmt", [29, 31, 36, 38, 40, 47, 33, 34])
def test_rgba8_reference_pins_to_decode_sse(gpu_ctx, fmt):
    w, h = 61, 37
    img = synth.photo(w, h, seed=11)
    payload = _encode(gpu_ctx, fmt, 0, img)
    ints = gpu_ctx.decode_sse(payload, img, fmt, 0)
    got = gpu_ctx.compare(payload, img, fmt, 0)
    for c in got.compared():
        assert got.sse[c] * 255.0 ** 2 == pytest.approx(ints[c], rel=1e-9, abs=1e-6), (c, got.sse[c], ints[c])


def test_mask_and_psnr(gpu_ctx):
    w, h = 64, 48
    img = synth.photo(w, h, seed=5)
    payload = _encode(gpu_ctx, 36, 0, img)
    full = gpu_ctx.compare(payload, img, 36, 0, ssim=True)
    part = gpu_ctx.compare(payload, img, 36, 0, mask=(True, False, True, False), ssim=True)
    assert full.channels == 15 and part.channels == 0b0101
    for c in (0, 2):
        assert part.sse[c] == full.sse[c] and part.ssim[c] == full.ssim[c]
    for c in (1, 3):
        assert part.sse[c] == 0.0 and np.isnan(part.ssim[c])
    # an R8 layout compares R only, whatever the mask
    r8 = gpu_ctx.compare(_encode(gpu_ctx, 33, 0, img), img, 33, 0)
    assert r8.channels == 1
    mse = (full.sse[0] + full.sse[1] + full.sse[2]) / (3 * w * h)
    assert full.psnr([0, 1, 2]) == pytest.approx(10 * np.log10(1.0 / mse), rel=1e-12)
    assert full.psnr([0], peak=255.0) == pytest.approx(10 * np.log10(255.0 ** 2 * w * h / full.sse[0]), rel=1e-12)
    black = np.zeros((8, 8, 4), np.uint8)
    black[..., 3] = 255
    same = gpu_ctx.compare(_encode(gpu_ctx, 29, 0, black), black, 29, 0)
    assert same.sse == [0.0] * 4 and same.psnr() == float("inf")


def test_psnr_peaks_by_layout(gpu_ctx):
    src, ref = _source(33, 1, 16, 16)
    sn = gpu_ctx.compare(_encode(gpu_ctx, 33, 1, src), ref, 33, 1)
    assert sn.peak() == 2.0
    src, ref = _source(35, 4, 16, 16)
    hd = gpu_ctx.compare(_encode(gpu_ctx, 35, 4, src), ref, 35, 4)
    assert hd.peak() == max(hd.ref_max[:4]) > 1.0
    assert all(np.isnan(v) for v in gpu_ctx.compare(_encode(gpu_ctx, 35, 4, src), ref, 35, 4, ssim=True).ssim)


@pytest.mark.parametrize("w,h", [(10, 40), (40, 10), (3, 2)])
def test_ssim_below_eleven_is_nan(gpu_ctx, w, h):
    img = synth.photo(w, h, seed=2)
    got = gpu_ctx.compare(_encode(gpu_ctx, 29, 0, img), img, 29, 0, ssim=True)
    assert got.ssim_windows == 0 and all(np.isnan(v) for v in got.ssim)
    assert got.texels == w * h and got.channels == 15


def _chain(w, h, levels, seed):
    out = []
    for m in range(levels):
        out.append(synth.photo(max(1, w >> m), max(1, h >> m), seed=seed + m))
    return out


def test_texture_compare_mip_chain(gpu_ctx):
    imgs = _chain(64, 48, 4, 20)
    tex, src = Texture(64, 48, 0, 4), Texture(64, 48, 0, 4)
    for m, im in enumerate(imgs):
        assert tex.set_image(im, m) and src.set_image(im, m)
    assert tex.convert(Format.BC1_RGB, Type.UNorm)
    results, pooled = tex.compare(src)
    assert len(results) == 4
    ctx = api.Context(0)
    try:
        for m, (r, im) in enumerate(zip(results, imgs)):
            want = ctx.compare(tex.data(m), im, Format.BC1_RGB, Type.UNorm, mask=(1, 1, 1, 0), ssim=True)
            assert _bits(r) == _bits(want)
            assert r.channels == 0b0111        # BC1 RGB has no alpha
    finally:
        ctx.close()
    sse = sum(sum(r.sse[:3]) for r in results)
    n = sum(r.texels * 3 for r in results)
    assert pooled == pytest.approx(10 * np.log10(n / sse), rel=1e-12)
    with pytest.raises(ValueError):
        tex.compare(Texture(32, 48, 0, 4))


def test_texture_compare_cube(gpu_ctx):
    tex, src = Texture(Dimension.Cube, 32, 32), Texture(Dimension.Cube, 32, 32)
    faces = [synth.photo(32, 32, seed=40 + f) for f in range(6)]
    for f, im in enumerate(faces):
        assert tex.set_image(im, CubeFace(f)) and src.set_image(im, CubeFace(f))
    assert tex.convert(Format.BC3, Type.UNorm)
    results, pooled = tex.compare(src)
    assert len(results) == 6 and np.isfinite(pooled)
    for r in results:
        assert r.channels == 15 and not np.isnan(r.ssim[0])


def test_argument_errors(gpu_ctx):
    L, h = gpu_ctx._lib, gpu_ctx._h
    img = synth.photo(16, 16, seed=1)
    payload = _encode(gpu_ctx, 29, 0, img)
    res = api.CompareResult()

    def call(fmt=29, typ=0, blocks_bytes=None, w=16, hh=16, pix=0, pitch=64, flags=0, result=True, emap=None, cap=0):
        return L.cfhip_compare(h, fmt, typ, payload.ctypes.data, payload.nbytes if blocks_bytes is None else blocks_bytes,
                               w, hh, img.ctypes.data, pix, pitch, None, flags, ctypes.byref(res) if result else None,
                               emap, cap)
    assert call() == 0
    assert call(fmt=14) == api.E_UNSUPPORTED           # a standard format
    assert call(fmt=10) == api.E_UNSUPPORTED
    assert call(typ=1) == api.E_UNSUPPORTED            # BC1 SNorm: cfhip_query rejects it
    assert call(fmt=36, typ=4) == api.E_UNSUPPORTED
    assert call(blocks_bytes=payload.nbytes - 1) == api.E_INVALID
    assert call(w=0) == api.E_INVALID
    assert call(pix=3) == api.E_INVALID
    assert call(pitch=63) == api.E_INVALID
    assert call(flags=2) == api.E_INVALID
    assert call(result=False) == api.E_INVALID
    emap = (ctypes.c_float * 16)()
    assert call(emap=emap, cap=15) == api.E_CAPACITY
    assert call(emap=emap, cap=16) == 0
    with pytest.raises(ValueError):
        gpu_ctx.compare(payload, img[..., :3], 29, 0)
    with pytest.raises(ValueError):
        gpu_ctx.compare(payload, img.astype(np.float64), 29, 0)
    with pytest.raises(api.CfhipError):
        gpu_ctx.compare(payload, img, 14, 0)


@pytest.mark.parametrize("fmt,typ", [(29, 0), (33, 1), (42, 0), (35, 4), (47, 0)],
                         ids=["rgba8", "r8-snorm", "rg16", "rgba16f", "astc"])
def test_4096(gpu_ctx, fmt, typ):
    w = h = 4096
    bw, bh, bs = api.query(fmt, typ)
    rng = np.random.default_rng(fmt * 10 + typ)
    payload = rng.integers(0, 256, ((h // bh + (h % bh > 0)) * (w // bw + (w % bw > 0)) * bs,), dtype=np.uint8)
    ref = synth.hdr_probe(w, h) if typ == 4 else synth.photo(w, h, seed=9)
    dec, bad = gpu_ctx.decode(payload, fmt, typ, w, h)
    layout, _ = api.decoded_layout(fmt, typ)
    want = R.compare(dec, layout, ref, (bw, bh), ssim=False)
    got = gpu_ctx.compare(payload, ref, fmt, typ, ssim=True, block_map=True)
    assert got.error_blocks == bad
    want["ssim"] = got.ssim                       # SSIM is pinned on the small surfaces above
    want["windows"] = got.ssim_windows
    _check_against_restatement(got, want)
    if typ != 4:
        assert got.ssim_windows == (w - 10) * (h - 10)
        assert all(-1.0 <= got.ssim[c] <= 1.0 for c in got.compared())
    assert _bits(gpu_ctx.compare(payload, ref, fmt, typ, ssim=True, block_map=True)) == _bits(got)
