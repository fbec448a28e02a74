"""cfhip_png_* without a GPU: the exports, the struct against the header's text, cfhip_png_bound against the twin's worst
case, every argument error and the order in which they are reported -- each returns before any device call, a NULL
context last -- the unsupported colour types and depths, zero sizes, cap one byte short, 2^31 filtered bytes from the
dimensions alone, and the Python surface."""
import ctypes
import os

import numpy as np
import pytest

import deflate_ref
import png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_png_bound", "cfhip_png_encode", "cfhip_png_encode_device", "cfhip_png_stage_ms")


def test_exports_and_struct(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    R = api.PngResult
    assert ctypes.sizeof(R) == 120 and tuple(n for n, _ in R._fields_) == png_ref.FIELDS
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 44, 48]
    assert _struct_fields("cfhip_png_result") == [("uint64_t", "bytes_out"), ("uint64_t", "idat_bytes"),
                                                  ("uint64_t", "filtered_bytes"), ("uint32_t", "rows_by_filter[5]"),
                                                  ("uint32_t", "idat_crc32"), ("cfhip_deflate_result", "deflate")]
    assert api.PNG_STAGES == ("filter",) + api.DEFLATE_STAGES + ("crc", "final") and len(api.PNG_STAGES) == 11
    assert (api.PNG_GREY, api.PNG_RGB, api.PNG_GREY_ALPHA, api.PNG_RGBA) == png_ref.COLOR_TYPES
    assert api.PNG_FILTERS == png_ref.FILTERS


def test_png_bound(hip_lib):
    from cuttlefish_amd import api
    for w, h in ((1, 1), (7, 1), (1, 7), (67, 29), (8192, 8192), (65535, 3)):
        for ct in png_ref.COLOR_TYPES:
            for depth in png_ref.DEPTHS:
                for cs in (0, 1):
                    n = h*(1 + w*png_ref.bpp(ct, depth))
                    want = 8 + 25 + (13 if cs else 0) + 12 + api.deflate_bound(n) + 12
                    assert api.png_bound(w, h, ct, depth, cs) == png_ref.png_bound(w, h, ct, depth, bool(cs)) == want
    # the twin's worst case: bytes no match search shrinks make every group a stored one, and the file still fits
    rng = np.random.default_rng(5)
    for w, h in ((67, 29), (200, 90)):
        noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        data, res = png_ref.encode(noise, png_ref.RGBA, 8, True)
        bound = api.png_bound(w, h, png_ref.RGBA, 8, 1)
        assert res["deflate"]["blocks_stored"] >= 1 and len(data) <= bound
        assert bound - len(data) <= 6 + 10*((res["filtered_bytes"] + 65535)//65536)
    # what the calls do not take has no bound
    for args in ((0, 5, 6, 8, 0), (5, 0, 6, 8, 0), (5, 5, 3, 8, 0), (5, 5, 1, 8, 0), (5, 5, 6, 4, 0), (5, 5, 6, 12, 0),
                 (5, 5, 6, 8, 2), (5, 5, 6, 8, -1)):
        assert api.png_bound(*args) == 0, args


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_errors_and_their_order(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    img = png_ref.image(5, 3, np.float32)
    bound = api.png_bound(5, 3, 6, 8, 0)
    out = np.full(bound + 8, 0xAB, np.uint8)
    res = (ctypes.c_uint64*15)()
    ok = dict(pixels=img.ctypes.data, pt=1, pitch=5*16, w=5, h=3, ct=6, depth=8, cs=0, out=out.ctypes.data, cap=bound,
              res=ctypes.addressof(res))

    def call(**kw):
        a = dict(ok, **kw)
        args = (None, a["pixels"], a["pt"], a["pitch"], a["w"], a["h"], a["ct"], a["depth"], a["cs"], a["out"], a["cap"], a["res"])
        if device:
            return hip_lib.cfhip_png_encode_device(*args, None)
        return hip_lib.cfhip_png_encode(*args)
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    # each error alone
    assert call(out=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(res=None) == api.E_INVALID and b"result is NULL" in err()
    assert call(pixels=None) == api.E_INVALID and b"pixels is NULL" in err()
    assert call(w=0) == api.E_INVALID and b"empty image" in err()
    assert call(h=0) == api.E_INVALID and b"empty image" in err()
    assert call(pt=3) == api.E_INVALID and b"pixel type" in err()
    assert call(cs=2) == api.E_INVALID and b"colour space" in err()
    assert call(ct=3) == api.E_UNSUPPORTED and b"palette" in err()
    for ct in (1, 5, 7, -1):
        assert call(ct=ct) == api.E_INVALID and b"colour type" in err()
    for depth in (1, 2, 4):
        assert call(depth=depth) == api.E_UNSUPPORTED and b"bit depth" in err()
    for depth in (0, 3, 12, 32):
        assert call(depth=depth) == api.E_INVALID and b"bit depth" in err()
    assert call(pitch=5*16 - 1) == api.E_INVALID and b"pitch" in err()
    assert call(cap=bound - 1) == api.E_CAPACITY and b"cfhip_png_bound" in err()
    assert call(cap=0) == api.E_CAPACITY
    # 2^31 filtered bytes or more, from the dimensions alone (no buffer of that size exists here)
    assert call(w=1 << 16, h=1 << 13, pitch=(1 << 16)*16, cap=1 << 40) == api.E_CAPACITY and b"2^31" in err()
    assert call(w=0xFFFFFFFF, h=0xFFFFFFFF, pitch=0xFFFFFFFF*16, depth=16, cap=1 << 62) == api.E_CAPACITY and b"2^31" in err()
    # the largest that is not: 2^31 - 1 filtered bytes needs its bound
    assert call(w=1, h=(1 << 31)//5, pitch=16, cap=1 << 20) == api.E_CAPACITY and b"cfhip_png_bound" in err()
    if device:
        assert call(pixels=img.ctypes.data + 4) == api.E_INVALID and b"aligned" in err()
        assert call(pitch=5*16 + 4) == api.E_INVALID and b"aligned" in err()
        assert call(res=ctypes.addressof(res) + 4) == api.E_INVALID and b"aligned" in err()
    # the order: of two errors the earlier one is reported
    order = [(dict(out=None), b"out is NULL"), (dict(res=None), b"result is NULL"), (dict(pixels=None), b"pixels is NULL"),
             (dict(w=0), b"empty image"), (dict(pt=9), b"pixel type"), (dict(cs=7), b"colour space"), (dict(ct=3), b"palette"),
             (dict(depth=4), b"bit depth"), (dict(pitch=1), b"pitch"),
             (dict(w=1 << 16, h=1 << 13, pitch=(1 << 16)*16), b"2^31"), (dict(cap=1), b"cfhip_png_bound")]
    for i, (first, text) in enumerate(order):
        for later, _ in order[i + 1:]:
            kw = dict(later, **first)
            if "w" in first and "w" in later:
                continue
            call(**kw)
            assert text in err(), (first, later, err())
    assert (out == 0xAB).all() and not any(res)
    assert hip_lib.cfhip_png_stage_ms(None, (ctypes.c_float*11)()) == api.E_INVALID


def test_python_surface():
    from cuttlefish_amd import Image, Texture, api
    for f in (api.png_bound, api.Context.png_encode, api.Context.png_encode_device, api.Context.png_result,
              api.Context.png_stage_ms, Image.save, Image.save_bytes, Texture.decoded_png):
        assert callable(f)
    img = Image(np.zeros((2, 2, 4), np.float32))
    assert img.save("picture.jpg") is False and img.save("picture") is False
    with pytest.raises(ValueError):
        img.save_bytes(color_type=3)
    with pytest.raises(ValueError):
        img.save_bytes(bit_depth=4)
    assert Texture(8, 8).decoded_png(0) is None
    assert deflate_ref.deflate_bound(63) == api.deflate_bound(63)
