"""cfhip_lz_size* and cfhip_rdo_target* without a GPU: the exports, the structs, and the argument errors, every one of
which returns before any device call (a NULL context is reported last)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import lzsize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_lz_size", "cfhip_lz_size_device", "cfhip_lz_slice_bytes", "cfhip_lz_stage_ms", "cfhip_rdo_target",
         "cfhip_rdo_target_device")


def test_exports_and_structs(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    assert ctypes.sizeof(api.LzSpan) == 16 and ctypes.sizeof(api.LzStats) == 48
    assert tuple(n for n, _ in api.LzStats._fields_) == lzsize_ref.FIELDS
    R = api.RdoTargetResult
    assert ctypes.sizeof(R) == 32
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("lambda16", 0), ("reached", 4), ("trials", 8), ("est_bytes_plain", 16), ("est_bytes_final", 24)]


def test_constants_have_their_twins():
    text = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "lzsize.h")).read()

    def const(name):
        return int(re.search(r"#define %s (\d+)u?\b" % name, text).group(1))
    assert (const("CFLZ_MIN"), const("CFLZ_MAX"), const("CFLZ_WINDOW"), const("CFLZ_CANDS"), const("CFLZ_CHUNK"),
            const("CFLZ_COSTBLK")) == (lzsize_ref.MIN, lzsize_ref.MAX, lzsize_ref.W, lzsize_ref.K, lzsize_ref.CHUNK,
                                       lzsize_ref.COSTBLK)
    assert const("CFLZ_LL") == 286 and const("CFLZ_DD") == 30 and const("CFLZ_HIST") == 320


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_lz_size_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    data = np.arange(64, dtype=np.uint8)
    out = api.LzStats()
    ctypes.memset(ctypes.addressof(out), 0xAB, ctypes.sizeof(out))

    def call(spans, n=None, out_ptr=ctypes.addressof(out)):
        arr = (api.LzSpan*max(len(spans), 1))()
        for i, (ptr, size) in enumerate(spans):
            arr[i].bytes, arr[i].n = ptr, size
        n = len(spans) if n is None else n
        if device:
            return hip_lib.cfhip_lz_size_device(None, arr, n, out_ptr, None)
        return hip_lib.cfhip_lz_size(None, arr, n, out_ptr)
    good = [(data.ctypes.data, 64)]
    assert call(good) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(good, out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call([(None, 5)]) == api.E_INVALID and b"span 0" in err()
    assert call(good + [(None, 1)]) == api.E_INVALID and b"span 1" in err()
    entry = hip_lib.cfhip_lz_size_device if device else hip_lib.cfhip_lz_size
    tail = (None,) if device else ()
    assert entry(None, None, 2, ctypes.addressof(out), *tail) == api.E_INVALID and b"spans is NULL" in err()
    # 2^31 bytes or more, in one span or in all
    assert call([(data.ctypes.data, 1 << 31)]) == api.E_CAPACITY
    assert call([(data.ctypes.data, (1 << 31) - 1)]) == api.E_INVALID and b"ctx is NULL" in err()
    assert call([(data.ctypes.data, 1 << 30), (None, 0), (data.ctypes.data, 1 << 30)]) == api.E_CAPACITY and b"2^31" in err()
    if device:
        assert call(good, out_ptr=ctypes.addressof(out) + 4) == api.E_INVALID and b"aligned" in err()
        assert call([]) == api.E_INVALID and b"ctx is NULL" in err()         # clearing the result needs the stream
    else:
        # an empty stream needs no context: all-zero stats
        assert call([]) == 0 and call([(None, 0), (data.ctypes.data, 0)]) == 0
        assert out.as_dict() == dict.fromkeys(lzsize_ref.FIELDS, 0)
        assert entry(None, None, 0, ctypes.addressof(out)) == 0
    assert hip_lib.cfhip_lz_slice_bytes(None, 65536) == 0
    assert hip_lib.cfhip_lz_stage_ms(None, (ctypes.c_float*5)()) == api.E_INVALID


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rdo_target_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    blk, out, src = np.zeros(16*8, np.uint8), np.zeros(16*8, np.uint8), np.zeros((16, 16, 4), np.uint8)
    stats = (api.RdoStats*2)()
    res = api.RdoTargetResult()

    def call(ratio=0.85, fmt=29, n=2, lam=32.0, result=True, params=True, stats_ok=True, **edit):
        s = (api.RdoSurface*2)()
        for i in range(2):
            s[i].blocks, s[i].blocks_bytes = blk.ctypes.data, blk.nbytes
            s[i].out, s[i].out_capacity = out.ctypes.data, out.nbytes
            s[i].width = s[i].height = 16
            s[i].pixels, s[i].pixel_type, s[i].row_pitch_bytes = src.ctypes.data, 0, 64
        for k, v in edit.items():
            setattr(s[1], k, v)
        p = api.make_rdo_ex_params(lam, None, row_above=True)
        args = [None, fmt, 0, s, n, ctypes.byref(p) if params else None, None,
                ctypes.addressof(stats) if stats_ok else None, ratio, ctypes.byref(res) if result else None]
        if device:
            return hip_lib.cfhip_rdo_target_device(*args, None)
        return hip_lib.cfhip_rdo_target(*args)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    for ratio in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(ratio) == api.E_INVALID and b"target_ratio" in err(), ratio
    for ratio in (1e-6, 0.5, 0.999):
        assert call(ratio) == api.E_INVALID and b"ctx is NULL" in err(), ratio
    assert call(result=False) == api.E_INVALID and b"result is NULL" in err()
    # the checks of cfhip_rdo_ex come first, in their order
    assert call(fmt=37) == api.E_UNSUPPORTED and b"RDO table" in err()
    assert call(0.0, lam=0.0) == api.E_INVALID and b"lambda" in err()
    assert call(0.0, width=0) == api.E_INVALID and b"empty surface" in err()
    assert call(out_capacity=out.nbytes - 1) == api.E_CAPACITY
    assert call(params=False) == api.E_INVALID and call(stats_ok=False) == api.E_INVALID
    # no surface: nothing to do, and the result says so
    res.trials = 9
    assert call(n=0) == 0 and res.as_dict() == dict(lambda16=0, reached=0, trials=0, est_bytes_plain=0, est_bytes_final=0)
    name = b"rdo_target_device" if device else b"rdo_target:"
    assert call(0.0) == api.E_INVALID and name in err()


def test_python_surface():
    from cuttlefish_amd import Texture, api
    for f in (api.Context.lz_size, api.Context.lz_size_device, api.Context.rdo_target, api.Context.rdo_target_device,
              Texture.packed_size, Texture.rdo_target):
        assert callable(f)
    assert inspect.signature(Texture.convert_rdo).parameters["target_ratio"].default is None
    t = Texture(8, 8)
    assert t.packed_size() is None and t.rdo_target() is None
