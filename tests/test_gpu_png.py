"""cfhip_png_encode* on the GPU against the definition, tests/png_ref.py: byte identity over every colour type, depth,
source type and the odd sizes, host form and device form (a pitch wider than tight, a source offset by one texel, a
stream of its own, a canary behind cap, the IDAT data on and off a word boundary); identical calls; rows of several
strides at odd output offsets; a stream of several slices and many CRC pieces; every filter; Image.save_bytes and
Texture.decoded_png."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image as PilImage

import png_ref as P
from cuttlefish_amd import Channel, ColorSpace, Format, Image, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

MATRIX = [(w, h, ct, d) for w, h in P.SIZES for ct in P.COLOR_TYPES for d in P.DEPTHS]


@pytest.fixture(scope="module")
def twins():
    """{(w, h, dtype name, colour type, depth, sRGB): (file, result)}, computed once"""
    cache = {}

    def get(w, h, dt, ct, depth, srgb):
        key = (w, h, np.dtype(dt).name, ct, depth, srgb)
        if key not in cache:
            cache[key] = P.encode(P.image(w, h, dt), ct, depth, srgb)
        return cache[key]
    return get


def _device_encode(ctx, img, ct, depth, cs, out_shift=0, stream=0, wide=1, lead=1):
    """png_encode_device of img embedded in a wider buffer behind `lead` texels -> (file, result dict, canary intact)"""
    import torch
    h, w = img.shape[:2]
    host = np.zeros((h, w + wide, 4), img.dtype)
    host[:, :w] = img
    flat = np.concatenate([np.zeros(lead*4, img.dtype), host.reshape(-1)])
    t = torch.from_numpy(flat.view(np.uint8) if img.dtype != np.uint8 else flat).to("cuda:0")
    tb = 4*img.dtype.itemsize
    cap = api.png_bound(w, h, ct, depth, cs)
    out = torch.full((cap + out_shift + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    res = torch.zeros(15, dtype=torch.int64, device="cuda:0")
    ctx.png_encode_device(t.data_ptr() + lead*tb, api.pixel_type_of(img), (w + wide)*tb, w, h, out.data_ptr() + out_shift, cap,
                          res.data_ptr(), color_type=ct, bit_depth=depth, color_space=cs, stream=stream)
    if stream:
        torch.cuda.synchronize()
    o = out.cpu().numpy()
    r = api.PngResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    canary = (o[:out_shift] == 0xAB).all() and (o[out_shift + cap:] == 0xAB).all()
    return o[out_shift:out_shift + r["bytes_out"]].tobytes(), r, bool(canary)


@pytest.mark.parametrize("dt", P.DTYPES, ids=[np.dtype(d).name for d in P.DTYPES])
def test_host_form_equals_the_twin(gpu_ctx, twins, dt):
    for w, h, ct, depth in MATRIX:
        srgb = (w + ct + depth) % 3 == 0
        want, want_res = twins(w, h, dt, ct, depth, srgb)
        got = gpu_ctx.png_encode(P.image(w, h, dt), ct, depth, ColorSpace.sRGB if srgb else ColorSpace.Linear)
        assert got == want, (w, h, ct, depth)
        assert gpu_ctx.png_result() == want_res, (w, h, ct, depth)
    assert gpu_ctx.last_kernel_ms() > 0
    ms = gpu_ctx.png_stage_ms()
    assert tuple(ms) == api.PNG_STAGES and all(v >= 0 for v in ms.values()) and ms["filter"] > 0 and ms["crc"] > 0


@pytest.mark.parametrize("dt", P.DTYPES, ids=[np.dtype(d).name for d in P.DTYPES])
def test_device_form_equals_the_twin(gpu_ctx, twins, dt):
    import torch
    side = torch.cuda.Stream()
    for i, (w, h, ct, depth) in enumerate(MATRIX):
        srgb = (w + ct + depth) % 3 == 0
        want, want_res = twins(w, h, dt, ct, depth, srgb)
        # the IDAT data lies 41 or 54 bytes in: a shift of 3 or 2 puts it on a word (in place), 0 does not (moved)
        shift = (0, 3 if not srgb else 2)[i % 2]
        got, res, canary = _device_encode(gpu_ctx, P.image(w, h, dt), ct, depth, int(srgb), out_shift=shift,
                                          stream=side.cuda_stream if i % 3 == 0 else 0, wide=1 + i % 2, lead=1)
        assert got == want and res == want_res and canary, (w, h, ct, depth, shift)


def test_identical_calls_return_identical_bits(gpu_ctx):
    img = P.image(67, 29, np.float32, seed=3)
    a = _device_encode(gpu_ctx, img, P.RGBA, 16, 1)
    b = _device_encode(gpu_ctx, img, P.RGBA, 16, 1)
    assert a == b and a[2]
    assert gpu_ctx.png_encode(img, P.RGB, 8) == gpu_ctx.png_encode(img, P.RGB, 8)


def test_rows_of_several_strides_at_odd_offsets(gpu_ctx):
    # 300 pixels of 8 bytes: rows of 2400 bytes over the workgroup's four wavefronts, two trips each, at offsets y x 2401
    img = P.image(300, 40, np.float32, seed=1)
    want, want_res = P.encode(img, P.RGBA, 16, True)
    assert gpu_ctx.png_encode(img, P.RGBA, 16, ColorSpace.sRGB) == want and gpu_ctx.png_result() == want_res
    got, res, canary = _device_encode(gpu_ctx, img, P.RGBA, 16, 1)
    assert got == want and res == want_res and canary
    # and the widest row a single wavefront takes, beside the narrowest the workgroup splits
    for w in (256, 257):
        img = P.image(w, 9, np.float16, seed=w)
        assert gpu_ctx.png_encode(img, P.RGB, 8) == P.twin(img, P.RGB, 8), w


def test_several_slices_and_many_crc_pieces(gpu_ctx):
    # 1024 x 96 RGBA8: 393 312 filtered bytes -- seven groups, slices of 65536 bytes, some 24 CRC pieces of 16 KiB.  The
    # full twin is slow here: its filtered bytes, the encoder pinned to deflate_ref elsewhere, the CRCs and Pillow stand in
    img = synth.photo(1024, 96, seed=11)
    data, rows = P.filtered(img, P.RGBA, 8)
    assert len(data) == 393312
    before = gpu_ctx.lz_slice_bytes(65536)
    try:
        got = gpu_ctx.png_encode(img, P.RGBA, 8)
        res = gpu_ctx.png_result()
        moved, res2, canary = _device_encode(gpu_ctx, img, P.RGBA, 8, 0)       # the stream moved behind the header
    finally:
        gpu_ctx.lz_slice_bytes(before)
    body = gpu_ctx.deflate(np.frombuffer(data, np.uint8))
    chunks = P.read_chunks(got)                                                 # every chunk's CRC
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert zlib.decompress(chunks[1][1]) == data and chunks[1][1] == body
    assert res["rows_by_filter"] == rows and res["idat_crc32"] == zlib.crc32(b"IDAT" + body)
    assert res["idat_bytes"] == len(body) and res["filtered_bytes"] == len(data) and res["bytes_out"] == len(got)
    assert res["deflate"] == gpu_ctx.deflate_result()
    assert moved == got and res2 == res and canary
    assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(got))), img)


def test_every_filter(gpu_ctx):
    img = P.five_filter_image()
    want, want_res = P.encode(img, P.GREY, 8)
    assert gpu_ctx.png_encode(img, P.GREY, 8) == want
    res = gpu_ctx.png_result()
    assert res["rows_by_filter"] == want_res["rows_by_filter"] and all(res["rows_by_filter"])
    zeros = np.zeros((6, 300, 4), np.float16)
    assert gpu_ctx.png_encode(zeros, P.RGBA, 16) == P.twin(zeros, P.RGBA, 16)
    assert gpu_ctx.png_result()["rows_by_filter"] == [6, 0, 0, 0, 0]


def test_image_save_bytes(gpu_ctx, tmp_path):
    img = Image(synth.photo(70, 33, seed=4), ColorSpace.sRGB)
    assert img.flip_horizontal() and img.swizzle(Channel.Blue, Channel.Green, Channel.Red, Channel.Alpha)
    resident = img._last is not None and img._last[1] is img.pixels
    assert resident                                                            # the file is made from the op's buffer
    for ct, depth in ((None, 8), (P.RGBA, 16), (P.GREY_ALPHA, 8), (P.GREY, 16)):
        got = img.save_bytes(ct, depth)
        assert got == P.twin(img.pixels, P.RGBA if ct is None else ct, depth, True), (ct, depth)
    path = tmp_path/"picture.png"
    assert img.save(str(path)) and path.read_bytes() == img.save_bytes()
    assert img.save(str(tmp_path/"picture.tga")) is False and not (tmp_path/"picture.tga").exists()
    # an array assigned by the caller is uploaded; an RGBF image saves RGB
    img.pixels = np.ascontiguousarray(img.pixels[::-1])
    assert img.save_bytes() == P.twin(img.pixels, P.RGBA, 8, True)
    normal = Image(synth.photo(40, 20, seed=6)).create_normal_map()
    assert normal.rgbf and normal.save_bytes() == P.twin(normal.pixels, P.RGB, 8, False)
    assert np.array_equal(np.asarray(PilImage.open(io.BytesIO(normal.save_bytes()))),
                          P.quantise(normal.pixels, 8)[..., :3])


@pytest.mark.parametrize("fmt", [Format.BC1_RGB, Format.ASTC_6x6], ids=["BC1", "ASTC6x6"])
def test_texture_decoded_png(gpu_ctx, fmt):
    mips = 7
    tex = Texture(64, 64, mip_levels=mips, color_space=ColorSpace.sRGB if fmt == Format.BC1_RGB else ColorSpace.Linear)
    for m in range(mips):
        assert tex.set_image(synth.photo(tex.width(m), tex.height(m), seed=20 + m), m)
    assert tex.convert(fmt, Type.UNorm, Quality.Low)
    srgb = fmt == Format.BC1_RGB
    for mip, depth in ((0, 8), (0, 16), (mips - 1, 8), (mips - 1, 16)):
        assert (tex.width(mip), tex.height(mip)) == ((64, 64) if mip == 0 else (1, 1))
        got = tex.decoded_png(mip, bit_depth=depth)
        assert got == P.twin(tex.decode_image(mip), P.RGBA, depth, srgb), (mip, depth)
    with pytest.raises(ValueError):
        tex.decoded_png(0, bit_depth=4)
