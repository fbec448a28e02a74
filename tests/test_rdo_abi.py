"""The rate-distortion entry points of the C-ABI without a GPU: exports, the structs, the supported table, and the
argument errors, every one of which returns before any device call -- on whichever surface of the call it sits."""
import ctypes

import numpy as np

import rdo_ref

NAMES = ("cfhip_rdo_supported", "cfhip_rdo", "cfhip_rdo_device")


def test_exports_structs_and_abi_version(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    assert ctypes.sizeof(api.RdoParams) == 16 and api.RdoParams.max_sse_increase.offset == 4
    # pointer + size_t, pointer + size_t, two uint32, pointer, int (+ padding), size_t
    assert ctypes.sizeof(api.RdoSurface) == 64
    assert (api.RdoSurface.out.offset, api.RdoSurface.width.offset, api.RdoSurface.pixels.offset,
            api.RdoSurface.pixel_type.offset, api.RdoSurface.row_pitch_bytes.offset) == (16, 32, 40, 48, 56)
    assert ctypes.sizeof(api.RdoStats) == 48
    assert [n for n, _ in api.RdoStats._fields_] == ["blocks", "blocks_changed", "sse_before", "sse_after",
                                                     "bits_before", "bits_after"]
    for name in ("rdo", "rdo_device"):
        assert hasattr(api.Context, name)
    from cuttlefish_amd import Texture
    assert hasattr(Texture, "convert_rdo") and hasattr(Texture, "rdo_stats")


def test_supported_table(hip_lib):
    from cuttlefish_amd import api
    listed = {(29, 0), (30, 0), (31, 0), (32, 0), (33, 0), (34, 0), (36, 0)}      # BC1_RGB .. BC5 and BC7, UNorm
    assert set(rdo_ref.TABLE) == listed
    got = {(f, t) for f in range(-1, 70) for t in range(-1, 8) if hip_lib.cfhip_rdo_supported(f, t)}
    assert got == listed
    assert api.rdo_supported(api.Format.BC7) and not api.rdo_supported(api.Format.BC6H, api.Type.UFloat)
    assert not api.rdo_supported(api.Format.BC4, api.Type.SNorm)
    assert not api.rdo_supported(api.Format.ETC2_R8G8B8) and not api.rdo_supported(api.Format.ASTC_4x4)
    assert not api.rdo_supported(api.Format.PVRTC1_RGBA_4BPP) and not api.rdo_supported(api.Format.R8G8B8A8)
    # block sizes of the table are the library's
    for (f, t), (bs, _, splices) in rdo_ref.TABLE.items():
        assert api.query(f, t) == (4, 4, bs)
        assert all(0 <= a < b <= bs for a, b in splices) and len(set(splices)) == len(splices)


class _Call:
    """cfhip_rdo / _device without a context on n BC1 16x16 surfaces with RGBA8 sources; `edit` changes surface k"""

    def __init__(self, lib, device):
        from cuttlefish_amd import api
        self.api, self.lib, self.device = api, lib, device
        self.blk = np.zeros(16*8, np.uint8)
        self.out = np.zeros(16*8, np.uint8)
        self.src = np.zeros((16, 16, 4), np.uint8)
        self.stats = (api.RdoStats*4)()

    def surfaces(self, n=3, k=None, **edit):
        s = (self.api.RdoSurface*max(n, 1))()
        for i in range(n):
            s[i].blocks, s[i].blocks_bytes = self.blk.ctypes.data, self.blk.nbytes
            s[i].out, s[i].out_capacity = self.out.ctypes.data, self.out.nbytes
            s[i].width = s[i].height = 16
            s[i].pixels, s[i].pixel_type, s[i].row_pitch_bytes = self.src.ctypes.data, 0, 64
        if k is not None:
            for name, v in edit.items():
                setattr(s[k], name, v)
        return s

    def __call__(self, fmt=29, typ=0, s=None, n=3, lam=1.0, cap=0xFFFFFFFF, reserved=0, params=True, stats=True,
                 stats_off=0, ctx=None):
        s = self.surfaces(n) if s is None else s
        p = self.api.make_rdo_params(lam, cap)
        p.reserved[1] = reserved
        pp = ctypes.byref(p) if params else None
        st = ctypes.c_void_p(ctypes.addressof(self.stats) + stats_off) if stats else None
        if self.device:
            return self.lib.cfhip_rdo_device(ctx, fmt, typ, s, n, pp, None, st, None)
        return self.lib.cfhip_rdo(ctx, fmt, typ, s, n, pp, None, st)


def test_empty_call_unsupported_pairs_and_null_ctx_last(hip_lib):
    from cuttlefish_amd import api
    for device in (False, True):
        call = _Call(hip_lib, device)
        # n == 0 does nothing, so it needs no context -- and no table, parameters or statistics either
        assert call(n=0) == 0
        if device:
            assert hip_lib.cfhip_rdo_device(None, 36, 0, None, 0, None, None, None, None) == 0
        else:
            assert hip_lib.cfhip_rdo(None, 36, 0, None, 0, None, None, None) == 0
        # a faultless call: only the context is missing, and that is said last
        assert call() == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        # everything outside the table: before everything, even n == 0
        for fmt in list(range(0, 29)) + [35] + list(range(37, 64)):
            for n in (0, 3):
                assert call(fmt=fmt, n=n) == api.E_UNSUPPORTED, fmt
        for fmt, typ in ((29, 1), (33, 1), (34, 1), (36, 4), (35, 4), (35, 5), (32, 2)):
            assert call(fmt=fmt, typ=typ) == api.E_UNSUPPORTED, (fmt, typ)
        assert b"RDO table" in hip_lib.cfhip_last_error(None)
        # an argument error outranks the missing context
        for lam in (0.0, -1.0, 1024.5, float("nan"), float("inf")):
            assert call(lam=lam) == api.E_INVALID and b"lambda" in hip_lib.cfhip_last_error(None), lam
        assert call(lam=1024.0) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        assert call(lam=1e-6) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        assert call(cap=0) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        assert call(reserved=1) == api.E_INVALID and b"reserved" in hip_lib.cfhip_last_error(None)
        assert call(params=False) == api.E_INVALID and call(stats=False) == api.E_INVALID
        assert call(s=ctypes.cast(None, ctypes.POINTER(api.RdoSurface))) == api.E_INVALID
        assert call(stats_off=4) == api.E_INVALID and b"stats" in hip_lib.cfhip_last_error(None)


def test_every_surface_is_checked(hip_lib):
    from cuttlefish_amd import api
    for device in (False, True):
        call = _Call(hip_lib, device)
        for k in (0, 2):
            def bad(**edit):
                return call(s=call.surfaces(3, k, **edit))
            assert bad(row_pitch_bytes=63) == api.E_INVALID and b"pitch" in hip_lib.cfhip_last_error(None)
            assert b"surface %d" % k in hip_lib.cfhip_last_error(None)
            assert bad(width=0) == api.E_INVALID and bad(height=0) == api.E_INVALID
            assert bad(blocks=None) == api.E_INVALID and bad(out=None) == api.E_INVALID
            assert bad(pixels=None) == api.E_INVALID and b"NULL" in hip_lib.cfhip_last_error(None)
            assert bad(pixel_type=3) == api.E_INVALID and b"pixel type" in hip_lib.cfhip_last_error(None)
            assert bad(pixel_type=-1) == api.E_INVALID
            # a float source needs its wider rows
            assert bad(pixel_type=1) == api.E_INVALID and b"pitch" in hip_lib.cfhip_last_error(None)
            assert bad(out_capacity=call.out.nbytes - 1) == api.E_CAPACITY
            assert b"out_capacity" in hip_lib.cfhip_last_error(None)
            # a 17 x 16 surface has five blocks a row: the payload no longer fits
            assert bad(width=17, row_pitch_bytes=68, blocks_bytes=1 << 20) == api.E_CAPACITY
            # in place is a legal call: only the context is missing
            assert bad(out=call.blk.ctypes.data) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
            if device:
                assert bad(blocks_bytes=0) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
                # device sources are read with one aligned load per texel
                assert bad(pixels=call.src.ctypes.data + 2) == api.E_INVALID
                assert b"aligned" in hip_lib.cfhip_last_error(None)
                assert bad(row_pitch_bytes=66) == api.E_INVALID and b"aligned" in hip_lib.cfhip_last_error(None)
            else:
                assert bad(blocks_bytes=call.blk.nbytes - 1) == api.E_INVALID
                assert b"blocks_bytes" in hip_lib.cfhip_last_error(None)
                # a host source may have any pitch that holds a row
                assert bad(row_pitch_bytes=67) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)


def test_python_wrappers_without_a_device(hip_lib):
    import pytest
    from cuttlefish_amd import Format, Texture, Type, api
    ctx = api.Context.__new__(api.Context)          # no device: the checks below come before any device call
    ctx._lib, ctx._h = hip_lib, None
    blk = np.zeros(8, np.uint8)
    with pytest.raises(ValueError):
        ctx.rdo([blk, blk], [np.zeros((4, 4, 4), np.uint8)], 29, 0, 1.0)
    with pytest.raises(ValueError):
        ctx.rdo([blk], [np.zeros((4, 4, 3), np.uint8)], 29, 0, 1.0)
    assert ctx.rdo([], [], 29, 0, 1.0) == ([], [])
    with pytest.raises(api.CfhipError) as e:
        ctx.rdo([], [], 35, 4, 1.0)
    assert e.value.code == api.E_UNSUPPORTED
    with pytest.raises(api.CfhipError) as e:
        ctx.rdo([blk], [np.zeros((4, 4, 4), np.uint8)], 29, 0, 0.0)
    assert e.value.code == api.E_INVALID
    # Texture.convert_rdo answers False where convert() does and outside the table, before any device call
    t = Texture(16, 16)
    assert not t.convert_rdo(Format.BC7, Type.UNorm, rdo_lambda=1.0)              # images incomplete
    assert t.set_image(np.zeros((16, 16, 4), np.uint8))
    assert not t.convert_rdo(Format.BC7, Type.SNorm, rdo_lambda=1.0)              # illegal pair
    assert not t.convert_rdo(Format.BC6H, Type.UFloat, rdo_lambda=1.0)            # outside the table
    assert not t.convert_rdo(Format.ETC2_R8G8B8, Type.UNorm, rdo_lambda=1.0)
    assert not t.converted() and t.rdo_stats() is None and t.images_complete()
