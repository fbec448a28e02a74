"""The fused compare of the standard formats (cfhip_std_compare) on the MI355X against a float64 restatement fed with
the numpy twin's texels (tests/std_unpack_ref.py) and built from the plain-array pieces of tests/compare_ref.py, with
the tolerances of tests/test_gpu_compare.py; masks; bit-identical repeats and host / device forms; Texture.compare."""
import ctypes

import numpy as np
import pytest

import compare_ref as C
import oracle_lib as O
import std_unpack_ref as R
from cuttlefish_amd import Format, Texture, Type, api, make_params, synth
from test_oracle_stdpack import ALL_PAIRS, LEGAL

pytestmark = pytest.mark.gpu

UNORM, SNORM, UINT, INT, UFLOAT, FLOAT = range(6)


def restate(tex, ref, fmt, typ, mask=None, ssim=False):
    """the metrics of cfhip_std_compare in float64 from unpacked texels (h, w, 4) float32"""
    d, r = tex.astype(np.float64), C.reference(ref)
    h, w = r.shape[:2]
    stored = {c for c, _, _ in R.fields(fmt)}
    cm = sum(1 << c for c in range(4) if c in stored and (mask is None or mask[c]))
    hdr = typ in (UFLOAT, FLOAT)
    nan = float("nan")
    out = {"sse": [0.0]*4, "log_sse": [0.0]*4, "ref_max": [0.0]*4, "ssim": [nan]*4, "channels": cm, "windows": 0}
    ssim_on = ssim and typ in (UNORM, SNORM) and h >= 11 and w >= 11 and cm
    if ssim_on:
        out["windows"] = (h - 10)*(w - 10)
    for c in range(4):
        if not (cm >> c) & 1:
            continue
        e = d[:, :, c] - r[:, :, c]
        out["sse"][c] = float((e*e).sum())
        out["ref_max"][c] = float(r[:, :, c].max())
        if hdr:
            lg = np.log2(np.maximum(d[:, :, c], C.TINY)) - np.log2(np.maximum(r[:, :, c], C.TINY))
            out["log_sse"][c] = float((lg*lg).sum())
        else:
            out["log_sse"][c] = nan
        if ssim_on:
            out["ssim"][c] = C.ssim_channel(d[:, :, c], r[:, :, c], 2.0 if typ == SNORM else 1.0)
    return out


def check(got, want):
    for c in range(4):
        if (want["channels"] >> c) & 1:
            print("channel", c, "sse", got.sse[c], want["sse"][c], "log", got.log_sse[c], want["log_sse"][c], "ssim",
                  got.ssim[c], want["ssim"][c], "max", got.ref_max[c], want["ref_max"][c])
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
            assert got.sse[c] == 0.0 and got.ref_max[c] == 0.0 and got.log_sse[c] == 0.0 and np.isnan(got.ssim[c])
    assert got.channels == want["channels"]
    assert got.ssim_windows == want["windows"]
    assert got.error_blocks == 0 and got.block_errors is None


def bits(r):
    return (r.texels, r.error_blocks, r.channels, r.ssim_windows,
            np.array(r.sse + r.log_sse + r.ssim + r.ref_max).tobytes())


def source(typ, w, h, seed=3):
    """(what the packer takes, the reference the metrics read)"""
    if typ in (UFLOAT, FLOAT):
        # float32 values between the halves: a 16-bit Float conversion is lossy too
        img = synth.hdr_probe(w, h, seed=seed, signed=typ == FLOAT).astype(np.float32)*np.float32(1.0003)
        return img, img
    img = synth.photo(w, h, seed=seed)
    if typ == SNORM:
        f = (img.astype(np.float32)/255.0)*2.0 - 1.0
        return f, f
    if typ in (UINT, INT):
        f = img.astype(np.float32)*np.float32(1.7) - np.float32(60.0 if typ == INT else 0.0)
        return f, f
    return img, img


def device_compare(ctx, payload, ref, fmt, typ, mask=None, ssim=True, offset=0, stream=None):
    torch = pytest.importorskip("torch")
    h, w = ref.shape[:2]
    host = np.zeros(offset + payload.size, np.uint8)
    host[offset:] = payload
    d_pix = torch.from_numpy(host).cuda()
    d_ref = torch.from_numpy(np.ascontiguousarray(ref).view(np.uint8).reshape(-1)).cuda()
    d_res = torch.zeros(ctypes.sizeof(api.CompareResult), dtype=torch.uint8, device="cuda")
    pix = {np.uint8: 0, np.float32: 1, np.float16: 2}[ref.dtype.type]
    torch.cuda.synchronize()
    ctx.compare_std_device(d_pix.data_ptr() + offset, fmt, typ, w, h, d_ref.data_ptr(), pix, ref.strides[0],
                           d_res.data_ptr(), mask=mask, ssim=ssim,
                           stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    res = api.CompareResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    return api.Comparison(res, api.Layout.RGBA32F, None, typ=typ)


@pytest.mark.parametrize("fmt,typ", ALL_PAIRS)
def test_compare_matches_restatement(gpu_ctx, fmt, typ):
    torch = pytest.importorskip("torch")
    w, h = 37, 61                                        # ragged: five workgroups, the last one partial
    src, ref = source(typ, w, h)
    payload = gpu_ctx.encode([src], make_params(fmt, typ))[0]
    tex = R.unpack(payload, fmt, typ, w, h)
    want = restate(tex, ref, fmt, typ, ssim=True)
    got = gpu_ctx.compare_std(payload, ref, fmt, typ, ssim=True)
    assert got.texels == w*h and got.layout == api.Layout.RGBA32F
    assert gpu_ctx.last_kernel_name() == "cfhip_std_compare_kernel" and gpu_ctx.last_kernel_ms() > 0.0
    check(got, want)
    assert (got.ssim_windows > 0) == (typ in (UNORM, SNORM))
    # identical bits on a second call, through the device form, at an odd payload offset and on a caller's stream
    assert bits(gpu_ctx.compare_std(payload, ref, fmt, typ, ssim=True)) == bits(got)
    assert bits(device_compare(gpu_ctx, payload, ref, fmt, typ)) == bits(got)
    assert bits(device_compare(gpu_ctx, payload, ref, fmt, typ, offset=1 + fmt % 3, stream=torch.cuda.Stream())) == bits(got)
    # without the flag: no SSIM, the same sums
    plain = gpu_ctx.compare_std(payload, ref, fmt, typ)
    assert plain.sse == got.sse and plain.ssim_windows == 0 and all(np.isnan(v) for v in plain.ssim)


@pytest.mark.parametrize("fmt,typ", [(f, t) for f, t in ALL_PAIRS if t in (UNORM, SNORM, UINT, INT)])
def test_random_payload_against_restatement(gpu_ctx, fmt, typ):
    w, h = 523, 3                                        # 3*512 + 33 pixels
    rng = np.random.default_rng(7000 + 10*fmt + typ)
    payload = rng.integers(0, 256, size=w*h*LEGAL[fmt][typ], dtype=np.uint8)
    ref = (rng.random((h, w, 4), dtype=np.float32)*2 - 1).astype(np.float16 if fmt % 2 else np.float32)
    tex = R.unpack(payload, fmt, typ, w, h)
    got = gpu_ctx.compare_std(payload, ref, fmt, typ, ssim=True)
    check(got, restate(tex, ref, fmt, typ, ssim=True))   # a side below 11: no SSIM window
    assert bits(device_compare(gpu_ctx, payload, ref, fmt, typ)) == bits(got)


def test_masks_and_stored_channels(gpu_ctx):
    w, h = 48, 32
    img = synth.photo(w, h, seed=5)
    for fmt, typ, stored in ((14, 0, 15), (5, 0, 7), (11, 0, 3), (10, 0, 1), (1, 0, 3), (27, 4, 7), (19, 5, 1)):
        src, ref = source(typ, w, h, seed=6)
        payload = gpu_ctx.encode([src], make_params(fmt, typ))[0]
        tex = R.unpack(payload, fmt, typ, w, h)
        full = gpu_ctx.compare_std(payload, ref, fmt, typ, ssim=True)
        assert full.channels == stored
        check(full, restate(tex, ref, fmt, typ, ssim=True))
        m = (True, False, True, False)
        part = gpu_ctx.compare_std(payload, ref, fmt, typ, mask=m, ssim=True)
        assert part.channels == stored & 0b0101
        check(part, restate(tex, ref, fmt, typ, mask=m, ssim=True))
        for c in part.compared():
            assert part.sse[c] == full.sse[c] and (part.ssim[c] == full.ssim[c] or np.isnan(full.ssim[c]))
    # nothing compared: all zero, SSIM not run
    none = gpu_ctx.compare_std(gpu_ctx.encode([img], make_params(10, 0))[0], img, 10, 0, mask=(0, 1, 1, 1), ssim=True)
    assert none.channels == 0 and none.sse == [0.0]*4 and none.ssim_windows == 0


def test_peaks_and_psnr(gpu_ctx):
    w, h = 32, 32
    for typ, fmt in ((UNORM, 14), (SNORM, 14), (UINT, 22), (INT, 22), (FLOAT, 22), (UFLOAT, 28)):
        src, ref = source(typ, w, h, seed=8)
        got = gpu_ctx.compare_std(gpu_ctx.encode([src], make_params(fmt, typ))[0], ref, fmt, typ)
        if typ == UNORM:
            assert got.peak() == 1.0
        elif typ == SNORM:
            assert got.peak() == 2.0
        else:
            assert got.peak() == max(got.ref_max[c] for c in got.compared()) > 1.0
        total = sum(got.sse[c] for c in got.compared())
        if total:
            assert got.psnr() == pytest.approx(
                10*np.log10(got.peak()**2*w*h*len(got.compared())/total), rel=1e-12)


def test_argument_errors(gpu_ctx):
    L, hd = gpu_ctx._lib, gpu_ctx._h
    img = synth.photo(16, 16, seed=1)
    payload = gpu_ctx.encode([img], make_params(14, 0))[0]
    res = api.CompareResult()

    def call(fmt=14, typ=0, nbytes=None, w=16, hh=16, pix=0, pitch=64, flags=0, result=True):
        return L.cfhip_std_compare(hd, fmt, typ, payload.ctypes.data, payload.nbytes if nbytes is None else nbytes, w,
                                   hh, img.ctypes.data, pix, pitch, None, flags, ctypes.byref(res) if result else None)
    assert call() == 0 and res.texels == 256 and res.channels == 15 and res.sse[0] < 1e-9
    for fmt, typ in ((29, 0), (36, 0), (47, 4), (60, 0), (5, 5), (14, 4), (0, 0)):
        assert call(fmt=fmt, typ=typ) == api.E_UNSUPPORTED, (fmt, typ)
    assert call(nbytes=payload.nbytes - 1) == api.E_INVALID
    assert call(w=0) == api.E_INVALID and call(pix=3) == api.E_INVALID and call(pitch=63) == api.E_INVALID
    assert call(flags=2) == api.E_INVALID and call(result=False) == api.E_INVALID
    # the generic entry keeps refusing the standard formats
    assert L.cfhip_compare(hd, 14, 0, payload.ctypes.data, payload.nbytes, 16, 16, img.ctypes.data, 0, 64, None, 0,
                           ctypes.byref(res), None, 0) == api.E_UNSUPPORTED
    torch = pytest.importorskip("torch")
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def dev(ref_off=0, pitch=64, res_off=2048):
        return L.cfhip_std_compare_device(hd, 14, 0, ctypes.c_void_p(d.data_ptr()), 16, 16,
                                          ctypes.c_void_p(d.data_ptr() + 1024 + ref_off), 0, pitch, None, 0,
                                          ctypes.c_void_p(d.data_ptr() + res_off), None)
    assert dev() == 0
    assert dev(ref_off=2) == api.E_INVALID and dev(pitch=66) == api.E_INVALID and dev(res_off=2052) == api.E_INVALID


def _pooled_from_twin(tex, src_images, fmt, typ, chans):
    sse, n, peak = 0.0, 0, 0.0
    for (m, im) in enumerate(src_images):
        h, w = im.shape[:2]
        t = R.unpack(tex.data(m), fmt, typ, w, h).astype(np.float64)
        r = O.as_rgbaf(im).astype(np.float64)             # Texture.compare measures against the RGBAF image
        for c in chans:
            sse += float(((t[..., c] - r[..., c])**2).sum())
            peak = max(peak, float(r[..., c].max()))
        n += w*h*len(chans)
    if typ == UNORM:
        peak = 1.0
    elif typ == SNORM:
        peak = 2.0
    return float("inf") if sse == 0.0 else 10.0*float(np.log10(peak*peak*n/sse))


@pytest.mark.parametrize("fmt,typ,chans", [(5, 0, (0, 1, 2)), (14, 1, (0, 1, 2, 3)), (22, 5, (0, 1, 2, 3)),
                                           (28, 4, (0, 1, 2))], ids=["r5g6b5", "rgba8-snorm", "rgba16f", "rgb9e5"])
def test_texture_compare_standard_formats(gpu_ctx, fmt, typ, chans):
    w, h, levels = 64, 48, 3
    imgs = [source(typ, max(1, w >> m), max(1, h >> m), seed=20 + m)[0] for m in range(levels)]
    tex, src = Texture(w, h, 0, levels), Texture(w, h, 0, levels)
    for m, im in enumerate(imgs):
        assert tex.set_image(im, m) and src.set_image(im, m)
    assert tex.convert(Format(fmt), Type(typ))
    results, pooled = tex.compare(src)                    # ssim=True: NaN for the non-normalised types, no raise
    assert len(results) == levels
    for r in results:
        assert tuple(r.compared()) == chans
        assert np.isnan(r.ssim[0]) == (typ not in (UNORM, SNORM) or r.ssim_windows == 0)
    want = _pooled_from_twin(tex, imgs, fmt, typ, chans)
    print("pooled", pooled, want)
    assert np.isfinite(pooled) and pooled == pytest.approx(want, rel=1e-9)


def test_texture_compare_rgba8_of_an_rgba8_source_is_lossless(gpu_ctx):
    img = synth.photo(40, 24, seed=3)
    tex, src = Texture(40, 24), Texture(40, 24)
    assert tex.set_image(img) and src.set_image(img) and tex.convert(Format.R8G8B8A8, Type.UNorm)
    results, pooled = tex.compare(src)
    assert pooled == float("inf") and results[0].sse == [0.0]*4 and results[0].channels == 15
    assert all(abs(v - 1.0) < 1e-12 for v in results[0].ssim)
