"""cfhip_rdo_ex / cfhip_rdo_ex_device without a GPU: the exports, cfhip_rdo_ex_params, and the argument errors, every
one of which returns before any device call.  The checks shared with cfhip_rdo (tests/test_rdo_abi.py) are made
through the new entries as well."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_rdo_ex", "cfhip_rdo_ex_device")


def test_exports_struct_and_abi_version(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    P = api.RdoExParams
    assert ctypes.sizeof(P) == 32
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("struct_size", 0), ("lam", 4), ("max_sse_increase", 8), ("flags", 12), ("window_bytes", 16), ("reserved", 20)]
    assert api.RDO_ROW_ABOVE == 1
    p = api.make_rdo_ex_params(2.5)
    assert (p.struct_size, p.lam, p.max_sse_increase, p.flags, p.window_bytes, list(p.reserved)) == (
        32, 2.5, api.RDO_NO_CAP, 0, 0, [0, 0, 0])
    p = api.make_rdo_ex_params(1.0, 40, row_above=True, window_bytes=65536)
    assert (p.max_sse_increase, p.flags, p.window_bytes) == (40, 1, 65536)
    # the header's struct is the same 32 bytes, and the flag is declared there
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    assert "#define CFHIP_RDO_ROW_ABOVE 1u" in header and "#define CFHIP_ABI_VERSION 1\n" in header


class _Call:
    """cfhip_rdo_ex / _ex_device without a context on three BC1 16x16 surfaces with RGBA8 sources"""

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

    def __call__(self, fmt=29, typ=0, s=None, n=3, lam=1.0, params=True, stats=True, stats_off=0, reserved=None, **fields):
        s = self.surfaces(n) if s is None else s
        p = self.api.make_rdo_ex_params(lam, None, row_above=True)
        for name, v in fields.items():
            setattr(p, name, v)
        if reserved is not None:
            p.reserved[reserved] = 7
        pp = ctypes.byref(p) if params else None
        st = ctypes.c_void_p(ctypes.addressof(self.stats) + stats_off) if stats else None
        if self.device:
            return self.lib.cfhip_rdo_ex_device(None, fmt, typ, s, n, pp, None, st, None)
        return self.lib.cfhip_rdo_ex(None, fmt, typ, s, n, pp, None, st)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_field_of_the_params_is_checked(hip_lib, device):
    from cuttlefish_amd import api
    call = _Call(hip_lib, device)
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731

    def null_ctx(rc):
        return rc == api.E_INVALID and b"ctx is NULL" in err()
    # a faultless call: only the context is missing, and that is said last
    assert null_ctx(call()) and null_ctx(call(flags=0))
    for size in (0, 16, 28, 36):
        assert call(struct_size=size) == api.E_INVALID and b"struct_size" in err(), size
    # struct_size comes first: nothing behind a wrong size is looked at
    assert call(struct_size=16, lam=0.0, flags=6) == api.E_INVALID and b"struct_size" in err()
    for lam in (0.0, -1.0, 1024.5, float("nan"), float("inf")):
        assert call(lam=lam) == api.E_INVALID and b"lambda" in err(), lam
    assert call(lam=0.0, flags=2) == api.E_INVALID and b"lambda" in err()
    for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == api.E_INVALID and b"flags" in err(), flags
    assert call(flags=2, window_bytes=1) == api.E_INVALID and b"flags" in err()
    for window in (1, 63, (1 << 30) + 1, 0xFFFFFFFF):
        assert call(window_bytes=window) == api.E_INVALID and b"window_bytes" in err(), window
    for window in (0, 64, 256, 32768, 1 << 30):
        assert null_ctx(call(window_bytes=window)), window
    assert call(window_bytes=1, reserved=0) == api.E_INVALID and b"window_bytes" in err()
    for k in range(3):
        assert call(reserved=k) == api.E_INVALID and b"reserved" in err(), k
    assert null_ctx(call(max_sse_increase=0)) and null_ctx(call(lam=1024.0))
    # an argument error of the params outranks one of a surface, as in cfhip_rdo
    assert call(s=call.surfaces(3, 1, width=0), flags=2) == api.E_INVALID and b"flags" in err()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_checks_of_the_plain_entries_hold(hip_lib, device):
    from cuttlefish_amd import api
    call = _Call(hip_lib, device)
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # n == 0 does nothing: no context, table, parameters or statistics needed
    assert call(n=0) == 0 and call(n=0, params=False, stats=False) == 0
    for fmt in (0, 28, 35, 37, 59):
        for n in (0, 3):
            assert call(fmt=fmt, n=n) == api.E_UNSUPPORTED and b"RDO table" in err(), fmt
    assert call(fmt=33, typ=1) == api.E_UNSUPPORTED
    # outside the table outranks the params
    assert call(fmt=35, struct_size=0) == api.E_UNSUPPORTED
    assert call(params=False) == api.E_INVALID and call(stats=False) == api.E_INVALID
    assert call(s=ctypes.cast(None, ctypes.POINTER(api.RdoSurface))) == api.E_INVALID and b"NULL" in err()
    assert call(stats_off=4) == api.E_INVALID and b"stats" in err()
    for k in (0, 2):
        def bad(**edit):
            return call(s=call.surfaces(3, k, **edit))
        assert bad(row_pitch_bytes=63) == api.E_INVALID and b"pitch" in err() and b"surface %d" % k in err()
        assert bad(width=0) == api.E_INVALID and bad(pixels=None) == api.E_INVALID
        assert bad(pixel_type=3) == api.E_INVALID and b"pixel type" in err()
        assert bad(out_capacity=call.out.nbytes - 1) == api.E_CAPACITY and b"out_capacity" in err()
        assert bad(out=call.blk.ctypes.data) == api.E_INVALID and b"ctx is NULL" in err()
        if device:
            assert bad(pixels=call.src.ctypes.data + 2) == api.E_INVALID and b"aligned" in err()
        else:
            assert bad(blocks_bytes=call.blk.nbytes - 1) == api.E_INVALID and b"blocks_bytes" in err()
    assert b"rdo_ex_device" in err() if device else b"rdo_ex" in err()


def test_python_wrappers_choose_the_entry_without_a_device(hip_lib):
    from cuttlefish_amd import Texture, api
    ctx = api.Context.__new__(api.Context)          # no device: the checks below come before any device call
    ctx._lib, ctx._h = hip_lib, None
    blk, src = np.zeros(8, np.uint8), np.zeros((4, 4, 4), np.uint8)
    assert ctx._rdo_entry(False, 1.0, None, False, None)[0] is hip_lib.cfhip_rdo
    assert ctx._rdo_entry(True, 1.0, None, False, None)[0] is hip_lib.cfhip_rdo_device
    entry, p = ctx._rdo_entry(False, 1.0, 9, True, None)
    assert entry is hip_lib.cfhip_rdo_ex and (p.flags, p.window_bytes, p.max_sse_increase) == (1, 0, 9)
    entry, p = ctx._rdo_entry(True, 1.0, None, False, 4096)
    assert entry is hip_lib.cfhip_rdo_ex_device and (p.flags, p.window_bytes) == (0, 4096)
    assert ctx.rdo([], [], 29, 0, 1.0, row_above=True) == ([], [])
    with pytest.raises(api.CfhipError) as e:
        ctx.rdo([blk], [src], 29, 0, 1.0, row_above=True, window_bytes=8)
    assert e.value.code == api.E_INVALID and "window_bytes" in str(e.value)
    with pytest.raises(api.CfhipError) as e:
        ctx.rdo([blk], [src], 35, 4, 1.0, row_above=True)
    assert e.value.code == api.E_UNSUPPORTED
    import inspect
    for f in (api.Context.rdo, api.Context.rdo_device, Texture.convert_rdo):
        sig = inspect.signature(f).parameters
        assert sig["row_above"].default is False and sig["window_bytes"].default is None, f
