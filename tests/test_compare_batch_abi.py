"""The batched compare entry points of the C-ABI without a GPU: exports, the struct, and the argument errors, every
one of which returns before any device call -- on whichever surface of the call it sits."""
import ctypes

import numpy as np

NAMES = ("cfhip_compare_batch", "cfhip_compare_batch_device")


def test_exports_and_abi_version(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    # two pointers + size_t, two uint32, pointer + size_t, pointer + size_t
    assert ctypes.sizeof(api.CompareSurface) == 56
    assert api.CompareSurface.ref.offset == 24 and api.CompareSurface.block_errors.offset == 40
    assert hasattr(api.Context, "compare_batch") and hasattr(api.Context, "compare_batch_device")


class _Call:
    """cfhip_compare_batch / _device without a context on n BC1 16x16 surfaces with RGBA8 references; `edit`
    changes surface k"""

    def __init__(self, lib, device):
        from cuttlefish_amd import api
        self.api, self.lib, self.device = api, lib, device
        self.blk = np.zeros(16*8, np.uint8)
        self.ref = np.zeros((16, 16, 4), np.uint8)
        self.map = np.zeros(16, np.float32)
        self.res = (api.CompareResult*4)()

    def surfaces(self, n=3, k=None, **edit):
        s = (self.api.CompareSurface*max(n, 1))()
        for i in range(n):
            s[i].blocks, s[i].blocks_bytes = self.blk.ctypes.data, self.blk.nbytes
            s[i].width = s[i].height = 16
            s[i].ref, s[i].ref_pitch_bytes = self.ref.ctypes.data, 64
        if k is not None:
            for name, v in edit.items():
                setattr(s[k], name, v)
        return s

    def __call__(self, fmt=29, typ=0, s=None, n=3, pix=0, flags=0, res=True, res_off=0, ctx=None):
        s = self.surfaces(n) if s is None else s
        r = ctypes.c_void_p(ctypes.addressof(self.res) + res_off) if res else None
        if self.device:
            return self.lib.cfhip_compare_batch_device(ctx, fmt, typ, s, n, pix, None, flags, r, None)
        return self.lib.cfhip_compare_batch(ctx, fmt, typ, s, n, pix, None, flags, r)


def test_empty_call_unsupported_pairs_and_null_ctx_last(hip_lib):
    from cuttlefish_amd import api
    for device in (False, True):
        call = _Call(hip_lib, device)
        # n == 0 does nothing, so it needs no context -- and no table either
        assert call(n=0) == 0
        if device:
            assert hip_lib.cfhip_compare_batch_device(None, 36, 0, None, 0, 1, None, 1, None, None) == 0
        else:
            assert hip_lib.cfhip_compare_batch(None, 36, 0, None, 0, 1, None, 1, None) == 0
        # a faultless call: only the context is missing, and that is said last
        assert call() == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        # standard formats, PVRTC, Unknown and the pairs cfhip_compare rejects: before everything, even n == 0
        for fmt in list(range(0, 29)) + list(range(57, 64)):
            for n in (0, 3):
                assert call(fmt=fmt, n=n) == api.E_UNSUPPORTED, fmt
        for fmt, typ in ((29, 1), (36, 4), (35, 0), (33, 4), (41, 2), (47, 1), (47, 5)):
            assert call(fmt=fmt, typ=typ) == api.E_UNSUPPORTED, (fmt, typ)
            lay = ctypes.c_int()
            assert hip_lib.cfhip_decoded_layout(fmt, typ, ctypes.byref(lay), None) != 0
        # an argument error outranks the missing context
        assert call(pix=3) == api.E_INVALID and b"pixel type" in hip_lib.cfhip_last_error(None)
        assert call(flags=2) == api.E_INVALID and b"flags" in hip_lib.cfhip_last_error(None)
        assert call(res=False) == api.E_INVALID
        assert call(s=ctypes.cast(None, ctypes.POINTER(api.CompareSurface))) == api.E_INVALID


def test_every_surface_is_checked(hip_lib):
    from cuttlefish_amd import api
    for device in (False, True):
        call = _Call(hip_lib, device)
        for k in (1, 2):
            def bad(**edit):
                return call(s=call.surfaces(3, k, **edit))
            assert bad(ref_pitch_bytes=63) == api.E_INVALID and b"pitch" in hip_lib.cfhip_last_error(None)
            assert b"surface %d" % k in hip_lib.cfhip_last_error(None)
            assert bad(width=0) == api.E_INVALID and bad(height=0) == api.E_INVALID
            assert bad(blocks=None) == api.E_INVALID and bad(ref=None) == api.E_INVALID
            fp = call.map.ctypes.data
            assert bad(block_errors=fp, block_errors_capacity=15) == api.E_CAPACITY
            assert b"block_errors_capacity" in hip_lib.cfhip_last_error(None)
            # enough room: only the context is missing
            assert bad(block_errors=fp, block_errors_capacity=16) == api.E_INVALID
            assert b"ctx is NULL" in hip_lib.cfhip_last_error(None)
            if device:
                assert bad(blocks_bytes=0) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
                # device references are read with one aligned load per texel, maps written as floats
                assert bad(ref=call.ref.ctypes.data + 2) == api.E_INVALID
                assert b"aligned" in hip_lib.cfhip_last_error(None)
                assert bad(ref_pitch_bytes=66) == api.E_INVALID and b"aligned" in hip_lib.cfhip_last_error(None)
                assert bad(block_errors=fp + 2, block_errors_capacity=16) == api.E_INVALID
                assert b"block_errors" in hip_lib.cfhip_last_error(None)
            else:
                assert bad(blocks_bytes=call.blk.nbytes - 1) == api.E_INVALID
                assert b"blocks_bytes" in hip_lib.cfhip_last_error(None)
                # a host reference may have any pitch that holds a row
                assert bad(ref_pitch_bytes=67) == api.E_INVALID and b"ctx is NULL" in hip_lib.cfhip_last_error(None)
        # the results are n structs of doubles: a pointer off by 4 is refused whatever n is
        assert call(res_off=4) == api.E_INVALID and b"results" in hip_lib.cfhip_last_error(None)
        # SSIM's size limit is a per-surface rule too (a 65536 x 65536 surface has 2^32 - ... windows: too many)
        big = call.surfaces(3, 2, width=70000, height=70000, ref_pitch_bytes=70000*4, blocks_bytes=1 << 40)
        assert call(s=big, flags=1) == api.E_INVALID and b"SSIM" in hip_lib.cfhip_last_error(None)


def test_python_wrapper_rejects_mixed_reference_types(hip_lib):
    import pytest
    from cuttlefish_amd import api
    ctx = api.Context.__new__(api.Context)          # no device: the checks below come before any call into the library
    ctx._lib, ctx._h = hip_lib, None
    blk = np.zeros(8, np.uint8)
    with pytest.raises(ValueError):
        ctx.compare_batch([blk, blk], [np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.float32)], 29, 0)
    with pytest.raises(ValueError):
        ctx.compare_batch([blk], [np.zeros((4, 4, 3), np.uint8)], 29, 0)
    with pytest.raises(ValueError):
        ctx.compare_batch([blk, blk], [np.zeros((4, 4, 4), np.uint8)], 29, 0)
    assert ctx.compare_batch([], [], 29, 0) == []
    with pytest.raises(api.CfhipError):
        ctx.compare_batch([], [], 14, 0)                # a standard format has no decoded layout
