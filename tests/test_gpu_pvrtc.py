"""PVRTC1 4 bpp on the MI355X: the encoder's payload byte-identical to the numpy twin (tests/pvrtc_ref.py) for both
formats, every level, small and rectangular sizes, three source types, negative pitch, alpha content and colour
masks; host and device entries and batches agree; the decoder and its fused SSE bit-exact; the Texture mirror."""
import numpy as np
import pytest

import pvrtc_ref as P
from cuttlefish_amd import Format, Quality, Texture, Type, api, make_params, synth
from cuttlefish_amd.texture import CubeFace, Dimension, FileType

pytestmark = pytest.mark.gpu

RGB, RGBA = Format.PVRTC1_RGB_4BPP, Format.PVRTC1_RGBA_4BPP
SIZES = [(1, 1), (4, 4), (8, 8), (16, 8), (8, 32), (64, 64), (256, 128)]


def content(w, h, kind, seed):
    img = synth.photo(max(w, 8), max(h, 8), seed=seed)[:h, :w].copy()
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        img[..., 3] = ((xx * 255) // max(w - 1, 1) + (yy * 97) // max(h, 1)) % 256
    elif kind == "cutout":
        img[..., 3] = np.where(((xx // 3) + (yy // 5)) % 3 == 0, 0, 255)
    else:
        img[..., 3] = 255
    return img


def as_type(img, t):
    if t == "u8":
        return img
    f = img.astype(np.float32) / np.float32(255)
    f[0, 0, 0] = np.float32(0.5 / 255)          # a value that rounds half-way
    return f.astype(np.float16) if t == "f16" else f


def surfaces(seed):
    kinds, types = ["opaque", "smooth", "cutout"], ["u8", "f16", "f32"]
    return [as_type(content(w, h, kinds[i % 3], seed + i), types[(i + seed) % 3]) for i, (w, h) in enumerate(SIZES)]


@pytest.mark.parametrize("fmt", [RGB, RGBA])
@pytest.mark.parametrize("quality", list(Quality))
def test_encoder_matches_numpy_twin(gpu_ctx, fmt, quality):
    imgs = surfaces(int(quality) + 7 * int(fmt))
    got = gpu_ctx.encode_pvrtc(imgs, make_params(fmt, Type.UNorm, quality))
    for img, g in zip(imgs, got):
        want = P.encode(img, int(fmt), int(quality))
        assert np.array_equal(g, want), (img.shape, img.dtype)


def test_batch_equals_one_by_one_and_negative_pitch(gpu_ctx):
    imgs = surfaces(3)
    p = make_params(RGBA, Type.UNorm, Quality.Normal)
    batch = gpu_ctx.encode_pvrtc(imgs, p)
    for img, b in zip(imgs, batch):
        assert np.array_equal(gpu_ctx.encode_pvrtc([img], p)[0], b)
    img = content(64, 32, "smooth", 11)
    flipped = img[::-1]                                   # rows bottom-up: negative pitch
    assert flipped.strides[0] < 0
    assert np.array_equal(gpu_ctx.encode_pvrtc([flipped], p)[0], P.encode(np.ascontiguousarray(flipped), 60, 2))


@pytest.mark.parametrize("mask", [(1, 0, 1, 1), (0, 1, 0, 0), (1, 1, 1, 0)])
def test_colour_mask(gpu_ctx, mask):
    img = content(32, 32, "smooth", 5)
    for fmt in (RGB, RGBA):
        got = gpu_ctx.encode_pvrtc([img], make_params(fmt, Type.UNorm, Quality.High, color_mask=mask))[0]
        assert np.array_equal(got, P.encode(img, int(fmt), 3, mask=mask))


def test_host_and_device_entries_agree(gpu_ctx):
    import torch
    imgs = [content(64, 64, "cutout", 2), content(16, 8, "opaque", 3), content(1, 1, "smooth", 4)]
    p = make_params(RGBA, Type.UNorm, Quality.Highest)
    host = gpu_ctx.encode_pvrtc(imgs, p)
    dev_in = [torch.from_numpy(im).to("cuda") for im in imgs]
    dev_out = [torch.zeros(h.size, dtype=torch.uint8, device="cuda") for h in host]
    gpu_ctx.encode_pvrtc_device([{"pixels": t.data_ptr(), "pixel_type": api.PixelType.RGBA8,
                                  "width": im.shape[1], "height": im.shape[0], "row_pitch_bytes": im.strides[0],
                                  "out": o.data_ptr(), "out_capacity": o.numel()}
                                 for im, t, o in zip(imgs, dev_in, dev_out)], p)
    torch.cuda.synchronize()
    for h, o in zip(host, dev_out):
        assert np.array_equal(h, o.cpu().numpy())


def _random_payload(rng, w, h):
    return rng.integers(0, 256, P.payload_size(w, h), dtype=np.uint8)


@pytest.mark.parametrize("w, h", [(1, 1), (4, 2), (8, 8), (16, 16), (32, 8), (8, 64), (256, 128), (128, 512)])
def test_decoder_and_sse_match_numpy(gpu_ctx, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    payload = _random_payload(rng, w, h)
    ref = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for fmt in (RGB, RGBA):
        want = P.decode(payload, w, h, int(fmt))
        assert np.array_equal(gpu_ctx.decode_pvrtc(payload, fmt, w, h), want)
        d = want.astype(np.int64) - ref
        assert gpu_ctx.decode_pvrtc_sse(payload, ref, fmt) == [int(v) for v in (d * d).sum(axis=(0, 1))]


def test_hand_vectors_on_gpu(gpu_ctx):
    from test_pvrtc_ref import blocks
    d = gpu_ctx.decode_pvrtc(blocks(0xFFFF8000, 0xE4E4E4E4), RGBA, 8, 8)
    assert list(d[0, :, 0]) == [0, 95, 159, 255] * 2
    d = gpu_ctx.decode_pvrtc(blocks(0xFFFF8001, 0xE4E4E4E4), RGBA, 8, 8)
    assert list(d[5, :, 3]) == [255, 255, 0, 255] * 2
    assert (gpu_ctx.decode_pvrtc(blocks(0x00007FFE, 0), RGBA, 8, 8).reshape(-1, 4) == [255, 255, 255, 238]).all()
    d = gpu_ctx.decode_pvrtc(blocks([0x8000FC00, 0x80008000, 0x80008000, 0x80008000], 0), RGBA, 8, 8)
    assert list(d[2, :, 0]) == [127, 191, 255, 191, 127, 63, 0, 63] == list(d[:, 2, 0])


def test_device_decode_entries(gpu_ctx):
    import torch
    rng = np.random.default_rng(9)
    payload = _random_payload(rng, 64, 32)
    ref = rng.integers(0, 256, (32, 64, 4), dtype=np.uint8)
    blk = torch.from_numpy(payload).to("cuda")
    out = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_pvrtc_device(blk.data_ptr(), RGBA, 64, 32, out.data_ptr(), 64 * 4)
    assert np.array_equal(out.cpu().numpy(), P.decode(payload, 64, 32))
    r = torch.from_numpy(ref).to("cuda")
    sse = torch.zeros(4, dtype=torch.int64, device="cuda")
    gpu_ctx.decode_pvrtc_sse_device(blk.data_ptr(), RGBA, 64, 32, r.data_ptr(), 64 * 4, sse.data_ptr())
    torch.cuda.synchronize()
    assert [int(v) for v in sse.cpu()] == P.sse(payload, ref)


@pytest.mark.parametrize("fmt", [RGB, RGBA])
def test_texture_convert_black_16(fmt):
    """TextureConvertTest's case (lib/test/TextureTest.cpp): a 16 x 16 black image"""
    t = Texture(Dimension.Dim2D, 16, 16)
    assert t.set_image(np.zeros((16, 16, 4), np.float32))
    assert t.convert(fmt, Type.UNorm)
    assert t.data_size() == 128
    with api.Context(0) as ctx:
        d = ctx.decode_pvrtc(t.data(), fmt, 16, 16)
    assert (d[..., :3] == 0).all() and ((d[..., 3] == 255).all() if fmt == RGB else True)


def test_texture_cube_mips_and_refusals():
    t = Texture(Dimension.Cube, 64, 64, mip_levels=Texture.allMipLevels)
    for face in range(6):
        for mip in range(t.mip_level_count()):
            s = 64 >> mip
            assert t.set_image(synth.photo(s, s, seed=face * 10 + mip).astype(np.float32) / 255, CubeFace(face), mip)
    assert t.convert(RGBA, Type.UNorm, Quality.Low)
    for face in CubeFace:
        assert [t.data_size(face, m) for m in range(t.mip_level_count())] == [2048, 512, 128, 32, 32, 32, 32]
    for bad in (Format.PVRTC1_RGB_2BPP, Format.PVRTC1_RGBA_2BPP, Format.PVRTC2_RGBA_2BPP, Format.PVRTC2_RGBA_4BPP):
        s = Texture(Dimension.Dim2D, 16, 16)
        s.set_image(np.zeros((16, 16, 4), np.float32))
        assert not s.convert(bad, Type.UNorm)
    s = Texture(Dimension.Dim2D, 24, 16)
    s.set_image(np.zeros((16, 24, 4), np.float32))
    assert not s.convert(RGB, Type.UNorm)


def test_texture_srgb_ktx_and_compare():
    img = synth.photo(32, 32, seed=4)
    src = Texture(Dimension.Dim2D, 32, 32, color_space=api.ColorSpace.sRGB)
    assert src.set_image(img)
    conv = Texture(Dimension.Dim2D, 32, 32, color_space=api.ColorSpace.sRGB)
    assert conv.set_image(img)
    assert conv.convert(RGBA, Type.UNorm, Quality.Normal)
    res, data = conv.save_bytes(FileType.KTX)
    assert int(res) == 0 and int.from_bytes(data[28:32], "little") == 0x8A57
    with pytest.raises(ValueError):
        conv.compare(src)                                   # SSIM is not offered for PVRTC
    _, psnr = conv.compare(src, ssim=False)
    want = api.psnr_from_sse(P.sse(conv.data(), P.to_rgba8(src.get_image()).astype(np.uint8)), 32 * 32, 4)
    assert abs(psnr - want) < 1e-9, (psnr, want)


def test_large_surface_sse_monotone_over_levels(gpu_ctx):
    img = synth.photo(2048, 2048, seed=1)
    last = None
    for q in Quality:
        p = gpu_ctx.encode_pvrtc([img], make_params(RGB, Type.UNorm, q))[0]
        s = sum(gpu_ctx.decode_pvrtc_sse(p, img, RGB)[:3])
        assert last is None or s <= last, (q, s, last)
        last = s
