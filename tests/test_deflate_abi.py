"""cfhip_deflate* without a GPU: the exports, the struct, the constants shared by the header, ctypes and the twin, the
bound, the empty stream, and the argument errors, every one of which returns before any device call (a NULL context is
reported last)."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import deflate_ref
import lzsize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_deflate_bound", "cfhip_deflate", "cfhip_deflate_device", "cfhip_deflate_stage_ms",
         "cfhip_deflate_code_lengths")


def test_exports_and_struct(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    R = api.DeflateResult
    assert ctypes.sizeof(R) == 72
    assert tuple(n for n, _ in R._fields_) == deflate_ref.FIELDS
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]
    # the header declares the same fields in the same order
    text = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    body = re.search(r"typedef struct cfhip_deflate_result \{(.*?)\} cfhip_deflate_result;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert tuple(names) == deflate_ref.FIELDS
    assert len(api.DEFLATE_STAGES) == 8 and api.DEFLATE_STAGES[:4] == api.LZ_STAGES[:4]


def test_constants_have_their_twins():
    text = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "deflate.h")).read()

    def const(name):
        return int(re.search(r"#define %s (\d+)u?\b" % name, text).group(1))
    assert (const("CFDF_STORED_SPLIT"), const("CFDF_LIMIT"), const("CFDF_CL_LIMIT")) == (
        deflate_ref.STORED_SPLIT, deflate_ref.LIMIT, deflate_ref.CL_LIMIT)
    assert const("CFDF_STAGES") == 8 and const("CFDF_HDR_WORDS")*32 >= 3 + 14 + 57 + 316*7
    order = re.search(r"df_cl_order\[19\] = \{([^}]*)\}", open(os.path.join(
        ROOT, "cuttlefish_amd", "csrc", "deflate.hip")).read()).group(1)
    assert tuple(int(v) for v in order.split(",")) == deflate_ref.CL_ORDER
    assert deflate_ref.STORED_SPLIT % lzsize_ref.CHUNK == 0 and lzsize_ref.COSTBLK <= 2*deflate_ref.STORED_SPLIT


def test_bound(hip_lib):
    from cuttlefish_amd import api
    for n in (0, 1, 65535, 65536, 65537, 200*1024, (1 << 31) - 1):
        assert api.deflate_bound(n) == deflate_ref.deflate_bound(n) == 11 + n + 10*((n + 65535)//65536)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    data = np.arange(64, dtype=np.uint8)
    out = np.full(api.deflate_bound(64) + 8, 0xAB, np.uint8)
    res = api.DeflateResult()

    def call(spans, n=None, out_ptr=out.ctypes.data, cap=out.size, res_ptr=ctypes.addressof(res)):
        arr = (api.LzSpan*max(len(spans), 1))()
        for i, (ptr, size) in enumerate(spans):
            arr[i].bytes, arr[i].n = ptr, size
        n = len(spans) if n is None else n
        if device:
            return hip_lib.cfhip_deflate_device(None, arr, n, out_ptr, cap, res_ptr, None)
        return hip_lib.cfhip_deflate(None, arr, n, out_ptr, cap, res_ptr)
    good = [(data.ctypes.data, 64)]
    assert call(good) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(good, out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(good, res_ptr=None) == api.E_INVALID and b"result is NULL" in err()
    assert call([(None, 5)]) == api.E_INVALID and b"span 0" in err()
    entry = hip_lib.cfhip_deflate_device if device else hip_lib.cfhip_deflate
    tail = (None,) if device else ()
    assert entry(None, None, 2, out.ctypes.data, out.size, ctypes.addressof(res), *tail) == api.E_INVALID
    assert b"spans is NULL" in err()
    assert call(good, cap=api.deflate_bound(64) - 1) == api.E_CAPACITY and b"cfhip_deflate_bound" in err()
    assert call(good, cap=api.deflate_bound(64)) == api.E_INVALID and b"ctx is NULL" in err()
    assert call([(data.ctypes.data, 1 << 31)], cap=1 << 40) == api.E_CAPACITY and b"2^31" in err()
    assert call([(data.ctypes.data, 1 << 30), (None, 0), (data.ctypes.data, 1 << 30)], cap=1 << 40) == api.E_CAPACITY
    assert (out == 0xAB).all()
    if device:
        assert call(good, out_ptr=out.ctypes.data + 2) == api.E_INVALID and b"aligned" in err()
        assert call([]) == api.E_INVALID and b"ctx is NULL" in err()
    else:
        # an empty stream needs no context: the fixed stream of an empty input
        assert call([]) == 0 and call([(None, 0), (data.ctypes.data, 0)]) == 0
        assert out[:11].tobytes() == deflate_ref.EMPTY and (out[11:] == 0xAB).all()
        assert zlib.decompress(deflate_ref.EMPTY) == b""
        assert res.as_dict() == deflate_ref.deflate(b"")[1]
        assert call([], cap=10) == api.E_CAPACITY
    assert hip_lib.cfhip_deflate_stage_ms(None, (ctypes.c_float*8)()) == api.E_INVALID
    assert hip_lib.cfhip_deflate_code_lengths(None, None, 2, 15, None) == api.E_INVALID


def test_python_surface():
    from cuttlefish_amd import Texture, api
    for f in (api.Context.deflate, api.Context.deflate_device, api.Context.deflate_stage_ms, api.deflate_bound,
              api.Context.deflate_code_lengths, Texture.pack, Texture.pack_result):
        assert callable(f)
    t = Texture(8, 8)
    assert t.pack() is None and t.pack_result() is None
