"""The standard-format unpack on the MI355X (csrc/std_unpack.hip) against the numpy twin (tests/std_unpack_ref.py),
bit for bit, for all 66 legal (format, type) pairs; the device entry; the loop closed through the product's own
packer; and Texture.decode_image for every family of formats convert() accepts."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pvrtc_ref as P
import std_unpack_ref as R
from cuttlefish_amd import CubeFace, Dimension, Format, Texture, Type, api, make_params, synth
from test_oracle_stdpack import ALL_PAIRS, LEGAL

pytestmark = pytest.mark.gpu

SUBDWORD = [(f, t) for f, t in ALL_PAIRS if LEGAL[f][t] in (1, 2, 3, 6)]
# one pair of every pixel size: 1, 2, 3, 4, 6, 8, 12, 16 bytes
BY_SIZE = [(10, 0), (5, 0), (12, 0), (18, 0), (21, 5), (22, 0), (25, 5), (26, 5)]


def same_bits(got, want):
    """bit for bit; where the twin has a NaN, any NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = (g != w) & ~nan
    assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])


def random_payload(fmt, typ, npix, seed=0):
    rng = np.random.default_rng(100000 + 100*fmt + typ + seed)
    return rng.integers(0, 256, size=npix*LEGAL[fmt][typ], dtype=np.uint8)


def test_by_size_lists_every_pixel_size():
    assert sorted(LEGAL[f][t] for f, t in BY_SIZE) == [1, 2, 3, 4, 6, 8, 12, 16]


@pytest.mark.parametrize("fmt,typ", ALL_PAIRS)
def test_ragged_surface_of_random_words(gpu_ctx, fmt, typ):
    w, h = 61, 37
    p = random_payload(fmt, typ, w*h)
    got = gpu_ctx.unpack(p, fmt, typ, w, h)
    same_bits(got, R.unpack(p, fmt, typ, w, h))
    assert gpu_ctx.last_kernel_name() == "cfhip_std_unpack_kernel" and gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("fmt,typ", [(f, t) for f, t in ALL_PAIRS if LEGAL[f][t] <= 2])
def test_every_16_bit_word(gpu_ctx, fmt, typ):
    p = np.arange(65536, dtype=np.uint32).astype("<u2").view(np.uint8)
    w, h = (256, 256) if LEGAL[fmt][typ] == 2 else (512, 256)
    same_bits(gpu_ctx.unpack(p, fmt, typ, w, h), R.unpack(p, fmt, typ, w, h))


@pytest.mark.parametrize("fmt,typ", [(17, 0), (18, 0), (17, 2), (18, 2), (27, 4), (28, 4)])
def test_every_value_of_the_fields_of_the_packed_32_bit_formats(gpu_ctx, fmt, typ):
    # 2048 words: every 11-bit value in the low field, every 10- / 9-bit value in the others, every top field value
    v = np.arange(2048, dtype=np.uint64)
    words = (v | ((v*7 + 3) % 2048 << np.uint64(11)) | ((v*5 + 1) % 1024 << np.uint64(22))).astype("<u4")
    p = np.concatenate([words, (words[::-1] >> np.uint32(1)) | (words << np.uint32(31))]).view(np.uint8)
    same_bits(gpu_ctx.unpack(p, fmt, typ, 64, 64), R.unpack(p, fmt, typ, 64, 64))


def device_unpack(ctx, payload, fmt, typ, w, h, offset=0, pad=0, out_shift=0, stream=None):
    """cfhip_std_unpack_device with the payload `offset` bytes into a buffer that ends where the payload ends, rows
    `pad` bytes longer than the texels, the output `out_shift` bytes into its buffer.  -> the texels"""
    torch = pytest.importorskip("torch")
    n = payload.size
    start = offset
    host = np.full(start + n, 0xA5, np.uint8)
    host[start:] = payload
    d_in = torch.from_numpy(host).cuda()
    assert (d_in.data_ptr() + start) % 4 == offset % 4
    pitch = w*16 + pad
    d_out = torch.full((out_shift + h*pitch,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.unpack_device(d_in.data_ptr() + start, fmt, typ, w, h, d_out.data_ptr() + out_shift, pitch,
                      stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    raw = d_out.cpu().numpy()
    rows = raw[out_shift:].reshape(h, pitch)
    assert np.all(raw[:out_shift] == 0xCD) and np.all(rows[:, w*16:] == 0xCD)      # padding untouched
    assert np.all(d_in.cpu().numpy() == host)
    return np.ascontiguousarray(rows[:, :w*16]).view(np.float32).reshape(h, w, 4)


@pytest.mark.parametrize("fmt,typ", ALL_PAIRS)
def test_partial_last_workgroup_and_the_end_of_the_payload(gpu_ctx, fmt, typ):
    # 3*512 + 33 pixels: a partial last workgroup; 3- and 6-byte pixels end 3 / 2 bytes into their last dword.  The
    # payload ends where its buffer ends; the kernel reads whole dwords only where all four bytes are payload.
    w, h = 523, 3
    p = random_payload(fmt, typ, w*h, seed=1)
    want = R.unpack(p, fmt, typ, w, h)
    same_bits(gpu_ctx.unpack(p, fmt, typ, w, h), want)
    same_bits(device_unpack(gpu_ctx, p, fmt, typ, w, h), want)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("fmt,typ", SUBDWORD)
def test_payload_at_odd_offsets(gpu_ctx, fmt, typ, offset):
    w, h = 131, 9                                        # 1179 pixels: two full workgroups and a partial one
    p = random_payload(fmt, typ, w*h, seed=2 + offset)
    got = device_unpack(gpu_ctx, p, fmt, typ, w, h, offset=offset, pad=48)
    same_bits(got, R.unpack(p, fmt, typ, w, h))


@pytest.mark.parametrize("fmt,typ", BY_SIZE)
def test_device_entry_stream_pitch_alignment(gpu_ctx, fmt, typ):
    torch = pytest.importorskip("torch")
    w, h = 77, 21
    p = random_payload(fmt, typ, w*h, seed=9)
    want = R.unpack(p, fmt, typ, w, h)
    host = gpu_ctx.unpack(p, fmt, typ, w, h)
    same_bits(host, want)
    s = torch.cuda.Stream()
    for kw in (dict(), dict(pad=16), dict(pad=48, stream=s), dict(pad=4, out_shift=4), dict(offset=1),
               dict(offset=2, pad=20, out_shift=12, stream=s)):
        got = device_unpack(gpu_ctx, p, fmt, typ, w, h, **kw)
        assert got.tobytes() == host.tobytes(), kw                               # host form == device form
    assert gpu_ctx.last_kernel_name() == "cfhip_std_unpack_kernel"


def test_argument_errors(gpu_ctx):
    L, hd = gpu_ctx._lib, gpu_ctx._h
    p = np.zeros(16*16*4, np.uint8)
    out = np.zeros((16, 16, 4), np.float32)

    def call(fmt=14, typ=0, nbytes=None, w=16, h=16, cap=None, pixels=True, dst=True):
        return L.cfhip_std_unpack(hd, fmt, typ, p.ctypes.data if pixels else None, p.nbytes if nbytes is None else nbytes,
                                  w, h, out.ctypes.data if dst else None, out.nbytes if cap is None else cap)
    assert call() == 0
    for fmt, typ in ((29, 0), (36, 0), (47, 0), (59, 0), (60, 0), (0, 0), (63, 0), (5, 5), (14, 5), (23, 0), (27, 0)):
        assert call(fmt=fmt, typ=typ) == api.E_UNSUPPORTED, (fmt, typ)
    for f in range(1, 29):
        for t in range(6):
            if t not in LEGAL[f]:
                assert call(fmt=f, typ=t, w=2, h=2) == api.E_UNSUPPORTED
    assert call(nbytes=p.nbytes - 1) == api.E_INVALID
    assert call(w=0) == api.E_INVALID and call(pixels=False) == api.E_INVALID and call(dst=False) == api.E_INVALID
    assert call(cap=out.nbytes - 1) == api.E_CAPACITY
    torch = pytest.importorskip("torch")
    d = torch.zeros(16*16*16 + 64, dtype=torch.uint8, device="cuda")

    def dev(fmt=14, typ=0, out_off=0, pitch=256):
        return L.cfhip_std_unpack_device(hd, fmt, typ, ctypes.c_void_p(d.data_ptr()), 16, 16,
                                         ctypes.c_void_p(d.data_ptr() + out_off), pitch, None)
    assert dev(fmt=29) == api.E_UNSUPPORTED
    assert dev(pitch=255) == api.E_INVALID            # below width * 16
    assert dev(pitch=258) == api.E_INVALID and dev(out_off=2) == api.E_INVALID      # floats need 4 bytes
    with pytest.raises(api.CfhipError) as e:
        gpu_ctx.unpack(p, Format.BC1_RGB, Type.UNorm, 16, 16)
    assert e.value.code == api.E_UNSUPPORTED
    # the generic entries keep their answer for the standard formats
    with pytest.raises(api.CfhipError):
        gpu_ctx.decode(p, 14, 0, 16, 16)


@pytest.mark.parametrize("fmt,typ", BY_SIZE)
def test_the_packer_reproduces_the_payload_2048(gpu_ctx, fmt, typ):
    w = h = 2048
    rng = np.random.default_rng(fmt)
    img = rng.random((h, w, 4), dtype=np.float32)
    if typ == 5:
        img = img*np.float32(8.0) - np.float32(4.0)
    prm = make_params(fmt, typ)
    payload = gpu_ctx.encode([img], prm)[0]
    tex = gpu_ctx.unpack(payload, fmt, typ, w, h)
    assert tex.shape == (h, w, 4) and tex.dtype == np.float32
    again = gpu_ctx.encode([tex], prm)[0]
    assert again.tobytes() == payload.tobytes()
    # a strip of it against the twin (the whole surface is slow in numpy)
    rows = 64
    same_bits(tex[-rows:], R.unpack(payload[-rows*w*LEGAL[fmt][typ]:], fmt, typ, w, rows))


# ---- Texture.decode_image ------------------------------------------------------------------------------

def _normalised(raw, layout):
    """Context.decode's array -> RGBAF by the rules cfhip_compare documents; absent channels 0, 0, 1"""
    h, w, n = raw.shape
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = 1.0
    L = api.Layout
    if layout == L.RGBA16F:
        out[..., :n] = raw.astype(np.float32)
        return out
    div = {L.RGBA8: 255.0, L.R8: 255.0, L.RG8: 255.0, L.R8_SNorm: 127.0, L.RG8_SNorm: 127.0, L.R16: 2047.0,
           L.RG16: 2047.0, L.R16_SNorm: 1023.0, L.RG16_SNorm: 1023.0}[layout]
    out[..., :n] = np.maximum(raw.astype(np.float64)/div, -1.0).astype(np.float32)
    return out


def _texture_source(typ, w, h, seed):
    if typ in (4, 5):
        return synth.hdr_probe(w, h, seed=seed, signed=typ == 5)
    img = synth.photo(w, h, seed=seed)
    if typ == 1:
        return (img.astype(np.float32)/255.0)*2.0 - 1.0
    if typ in (2, 3):
        return img.astype(np.float32) - (100.0 if typ == 3 else 0.0)
    return img


@pytest.mark.parametrize("fmt,typ", [(5, 0), (14, 1), (18, 2), (20, 3), (22, 5), (28, 4), (27, 4), (12, 0), (26, 5)])
def test_decode_image_standard_formats(gpu_ctx, fmt, typ):
    w, h = 40, 24
    tex = Texture(w, h)
    assert tex.set_image(_texture_source(typ, w, h, 5)) and tex.convert(Format(fmt), Type(typ))
    got = tex.decode_image()
    same_bits(got, R.unpack(tex.data(), fmt, typ, w, h))
    same_bits(got, R.unpack(O.std_pack(_texture_source(typ, w, h, 5), fmt, typ), fmt, typ, w, h))


@pytest.mark.parametrize("fmt,typ", [(29, 0), (33, 0), (33, 1), (34, 0), (34, 1), (41, 0), (41, 1), (42, 0), (42, 1),
                                     (35, 4), (36, 0), (40, 0), (47, 0), (47, 4)])
def test_decode_image_block_formats(gpu_ctx, fmt, typ):
    from test_gpu_decode import oracle_decode
    w, h = 40, 24
    tex = Texture(w, h)
    assert tex.set_image(_texture_source(typ, w, h, 6)) and tex.convert(Format(fmt), Type(typ), api.Quality.Lowest)
    raw, _ = oracle_decode(tex.data(), fmt, typ, w, h)
    layout, _ = api.decoded_layout(fmt, typ)
    if raw.dtype == np.uint16 and layout == api.Layout.RGBA16F:
        raw = raw.view(np.float16)
    got = tex.decode_image()
    want = _normalised(raw, layout)
    assert got.shape == (h, w, 4) and got.dtype == np.float32
    assert np.array_equal(got, want, equal_nan=True)


def test_decode_image_pvrtc(gpu_ctx):
    w = h = 32
    tex = Texture(w, h)
    assert tex.set_image(synth.photo(w, h, seed=8)) and tex.convert(Format.PVRTC1_RGBA_4BPP, Type.UNorm)
    want = _normalised(P.decode(tex.data(), w, h, P.RGBA), api.Layout.RGBA8)
    assert np.array_equal(tex.decode_image(), want)


def test_decode_image_cube_and_mips(gpu_ctx):
    tex = Texture(Dimension.Cube, 32, 32, 0, 3)
    assert tex.decode_image() is None                                  # not converted
    imgs = {}
    for f in range(6):
        for m in range(3):
            imgs[f, m] = synth.photo(32 >> m, 32 >> m, seed=10*f + m)
            assert tex.set_image(imgs[f, m], CubeFace(f), m)
    assert tex.convert(Format.R5G6B5, Type.UNorm)
    for f in range(6):
        for m in range(3):
            got = tex.decode_image(CubeFace(f), m)
            assert got.shape == (32 >> m, 32 >> m, 4)
            same_bits(got, R.unpack(O.std_pack(imgs[f, m], 5, 0), 5, 0, 32 >> m, 32 >> m))
    assert tex.decode_image(0) is None                                 # a cube needs a face
    assert tex.decode_image(CubeFace.PosX, 3) is None and tex.decode_image(CubeFace.PosX, 0, 1) is None
    arr = Texture(Dimension.Dim2D, 16, 8, 2, 2)
    for d in range(2):
        for m in range(2):
            assert arr.set_image(synth.photo(16 >> m, 8 >> m, seed=d + m), m, d)
    assert arr.convert(Format.BC4, Type.UNorm)
    assert arr.decode_image(1, 1).shape == (4, 8, 4) and arr.decode_image(0, 2) is None
    assert arr.decode_image(CubeFace.NegX) is None
