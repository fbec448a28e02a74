"""The batched decode entry points of the C-ABI without a GPU: exports, the output table, argument errors that
return before any device call, and the CPU proof of the division-free quotients the RGBA32F output uses."""
import ctypes

import numpy as np
import pytest

NAMES = ("cfhip_decode_batch", "cfhip_decode_batch_device", "cfhip_decode_out_supported")
U8 = ("RGBA8", "R8", "RG8")


def test_exports_and_abi_version(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    assert ctypes.sizeof(api.DecodeSurface) == 48


def test_out_supported_equals_the_table(hip_lib):
    from cuttlefish_amd import api
    P = api.PixelType
    legal = 0
    for fmt in range(29, 57):
        for typ in range(6):
            lay = ctypes.c_int()
            ok = hip_lib.cfhip_decoded_layout(fmt, typ, ctypes.byref(lay), None) == 0
            legal += ok
            name = api.Layout(lay.value).name if ok else ""
            want = {-1: ok, int(P.RGBA8): ok and name in U8, int(P.RGBA16F): ok and name == "RGBA16F",
                    int(P.RGBA32F): ok}
            for out, w in want.items():
                assert hip_lib.cfhip_decode_out_supported(fmt, typ, out) == int(w), (fmt, typ, out)
                assert api.decode_out_supported(fmt, typ, None if out < 0 else out) == bool(w)
            for out in (-2, 3, 99):
                assert hip_lib.cfhip_decode_out_supported(fmt, typ, out) == 0
    assert legal == 47
    for fmt in list(range(0, 29)) + list(range(57, 64)):
        for typ in range(6):
            for out in (-1, 0, 1, 2):
                assert hip_lib.cfhip_decode_out_supported(fmt, typ, out) == 0, (fmt, typ, out)


def test_argument_errors_return_before_any_device_call(hip_lib):
    """With no context at all every argument error is still reported as itself; a faultless call then says that
    the context is missing.  Nothing here can reach a device."""
    from cuttlefish_amd import api
    blk = np.zeros(16*4, np.uint8)
    out = np.zeros(8*8*16, np.uint8)

    def surf(w=8, h=8, pitch=32, cap=8*8*4, nbytes=64, bp=True, op=True):
        s = (api.DecodeSurface*1)()
        s[0].blocks = blk.ctypes.data if bp else None
        s[0].blocks_bytes = nbytes
        s[0].width, s[0].height = w, h
        s[0].out = out.ctypes.data if op else None
        s[0].out_pitch_bytes, s[0].out_capacity = pitch, cap
        return s

    def host(fmt=36, typ=0, pix=-1, s=None, n=1):
        return hip_lib.cfhip_decode_batch(None, fmt, typ, pix, surf() if s is None else s, n, None)

    def dev(fmt=36, typ=0, pix=-1, s=None, n=1):
        return hip_lib.cfhip_decode_batch_device(None, fmt, typ, pix, surf() if s is None else s, n, None, None)

    for call in (host, dev):
        assert call() == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        assert call(n=0) == api.E_INVALID                       # ... and an empty call without a context too
        for fmt in list(range(1, 29)) + list(range(57, 63)):
            assert call(fmt=fmt) == api.E_UNSUPPORTED, fmt
        assert call(typ=1) == api.E_UNSUPPORTED                 # BC7 SNorm
        assert call(pix=2) == api.E_UNSUPPORTED                 # BC7 -> RGBA16F
        assert call(fmt=33, typ=1, pix=0) == api.E_UNSUPPORTED  # BC4 SNorm -> RGBA8
        assert call(pix=7) == api.E_UNSUPPORTED
        assert hip_lib.cfhip_decode_batch(None, 36, 0, -1, None, 1, None) == api.E_INVALID
        assert b"surfaces is NULL" in hip_lib.cfhip_last_error(None)
        assert call(s=surf(w=0)) == api.E_INVALID and call(s=surf(h=0)) == api.E_INVALID
        assert call(s=surf(bp=False)) == api.E_INVALID and call(s=surf(op=False)) == api.E_INVALID
        assert call(s=surf(pitch=31)) == api.E_INVALID and b"pitch" in hip_lib.cfhip_last_error(None)
        assert call(pix=1, s=surf(pitch=127, cap=8*8*16)) == api.E_INVALID
    assert host(s=surf(nbytes=63)) == api.E_INVALID
    assert host(s=surf(cap=8*8*4 - 1)) == api.E_CAPACITY and b"out_capacity" in hip_lib.cfhip_last_error(None)
    assert host(pix=1, s=surf(pitch=128, cap=8*8*16 - 1)) == api.E_CAPACITY
    assert host(s=surf(pitch=40, cap=7*40 + 31)) == api.E_CAPACITY      # (h - 1) * pitch + row
    assert host(s=surf(pitch=40, cap=7*40 + 32)) == api.E_INVALID       # faultless: only the context is missing


@pytest.mark.parametrize("maxv,lo", [(2047, 0), (1023, -1024), (255, 0), (127, -128)])
def test_newton_quotient_is_the_rounded_quotient_for_the_decoders_divisors(maxv, lo):
    # std_unpack.h quot<MAX>: q = x*(1/MAX); q += fma(-q, MAX, x)*(1/MAX), as tests/test_std_unpack_ref.py models it,
    # against what Texture.decode_image computes: the double quotient rounded once to float
    x = np.arange(lo, maxv + 1, dtype=np.float64)
    r = np.float64(np.float32(1.0)/np.float32(maxv))
    q0 = (x*r).astype(np.float32).astype(np.float64)
    rem = (x - q0*maxv).astype(np.float32).astype(np.float64)
    t = rem*r
    want = (x/np.float64(maxv)).astype(np.float32)
    assert np.array_equal(want, x.astype(np.float32)/np.float32(maxv))
    for s in ((t + q0), np.nextafter(t + q0, np.inf), np.nextafter(t + q0, -np.inf)):
        assert np.array_equal(s.astype(np.float32), want)
