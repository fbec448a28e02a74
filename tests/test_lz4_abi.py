"""cfhip_lz4_* without a GPU: the exports, the structs against the header's text, the constants shared with the twin,
cfhip_lz4_bound, the argument errors, every one of which returns before any device call (a NULL context is reported
last), the empty frames, which need no context, and the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import lz4_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_lz4_bound", "cfhip_lz4_encode", "cfhip_lz4_encode_device", "cfhip_lz4_encode_stage_ms",
         "cfhip_lz4_decode", "cfhip_lz4_decode_device", "cfhip_lz4_decode_stage_ms")


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(decl.split(None, 1)[0], n.strip()) for decl in body.split(";") if decl.strip()
            for n in decl.split(None, 1)[1].split(",")]


def test_exports_and_structs(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    R = api.Lz4Result
    assert ctypes.sizeof(R) == 56 and tuple(n for n, _ in R._fields_) == lz4_ref.FIELDS
    assert _struct_fields("cfhip_lz4_result") == [("uint64_t", n) for n in lz4_ref.FIELDS]
    D = api.Lz4DecodeResult
    assert ctypes.sizeof(D) == 72 and tuple(n for n, _ in D._fields_) == lz4_ref.DECODE_FIELDS
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68]
    assert _struct_fields("cfhip_lz4_decode_result") == [("uint64_t", n) for n in lz4_ref.DECODE_FIELDS[:7]] + \
        [("uint32_t", n) for n in lz4_ref.DECODE_FIELDS[7:]]
    assert api.LZ4_ENCODE_STAGES == ("keys", "sort", "match", "parse", "plan", "offsets", "emit", "hash", "final")
    assert api.LZ4_DECODE_STAGES == ("chain", "blocks", "final")
    assert api.LZ4_CLASSES == lz4_ref.CLASSES and api.LZ4_BLOCK == lz4_ref.BLOCK and api.LZ4_MAGIC == lz4_ref.MAGIC
    assert api.LZ4_UNSUPPORTED == lz4_ref.E_UNSUPPORTED


def test_constants_have_their_twins():
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "lz4.h")).read()
    assert re.search(r"#define CFHIP_ABI_VERSION 1\b", header)
    names = ("OK", "HEADER", "UNSUPPORTED", "BLOCKS", "CHECKSUM", "SEQUENCE", "OFFSET", "SIZE")
    twin = (lz4_ref.OK, lz4_ref.E_HEADER, lz4_ref.E_UNSUPPORTED, lz4_ref.E_BLOCKS, lz4_ref.E_CHECKSUM, lz4_ref.E_SEQUENCE,
            lz4_ref.E_OFFSET, lz4_ref.E_SIZE)
    for name, value in zip(names, twin):
        assert int(re.search(r"CFHIP_LZ4_%s = (\d+)" % name, header).group(1)) == value
        macro = "CFLZ4_OK" if name == "OK" else "CFLZ4_E_" + name
        assert int(re.search(r"#define %s (\d+)u" % macro, shared).group(1)) == value
        assert lz4_ref.CLASSES[value] == name.lower()

    def macro(name):
        return int(re.search(r"#define %s (\w+)u" % name, shared).group(1), 0)
    assert macro("CFLZ4_BLOCK") == lz4_ref.BLOCK and macro("CFLZ4_HEADER") == lz4_ref.HEADER_BYTES
    assert macro("CFLZ4_FLG") == lz4_ref.FLG and macro("CFLZ4_BD") == lz4_ref.BD
    assert macro("CFLZ4_LAST_LITERALS") == lz4_ref.LAST_LITERALS and macro("CFLZ4_MATCH_MARGIN") == lz4_ref.MATCH_MARGIN
    assert (macro("CFLZ4_P1"), macro("CFLZ4_P2"), macro("CFLZ4_P3"), macro("CFLZ4_P4"), macro("CFLZ4_P5")) == \
        (lz4_ref.P1, lz4_ref.P2, lz4_ref.P3, lz4_ref.P4, lz4_ref.P5)
    assert int(re.search(r"#define CFLZ4_STAGES (\d+)", shared).group(1)) == 9
    assert int(re.search(r"#define CFLZ4_DSTAGES (\d+)", shared).group(1)) == 3


def test_lz4_bound(hip_lib):
    from cuttlefish_amd import api
    for n in (0, 1, 65535, 65536, 65537, 200*1024, (1 << 31) - 1, 1 << 40):
        assert api.lz4_bound(n) == lz4_ref.lz4_bound(n) == 19 + n + 8*((n + 65535)//65536)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_encode_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    data = np.arange(5000, dtype=np.uint8)
    out = np.full(api.lz4_bound(5000) + 8, 0xAB, np.uint8)
    res = api.Lz4Result()

    def call(n=5000, out_ptr=out.ctypes.data, cap=out.size, res_ptr=ctypes.addressof(res), spans=1, src=data.ctypes.data):
        span = (api.LzSpan*1)()
        span[0].bytes, span[0].n = src, n
        if device:
            return hip_lib.cfhip_lz4_encode_device(None, span, spans, out_ptr, cap, res_ptr, None)
        return hip_lib.cfhip_lz4_encode(None, span, spans, out_ptr, cap, res_ptr)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(res_ptr=None) == api.E_INVALID and b"result is NULL" in err()
    assert call(src=None) == api.E_INVALID and b"bytes is NULL" in err()
    assert call(cap=api.lz4_bound(5000) - 1) == api.E_CAPACITY and b"cfhip_lz4_bound" in err()
    assert call(n=1 << 31, cap=1 << 40) == api.E_CAPACITY and b"2^31" in err()
    if device:
        assert call(res_ptr=ctypes.addressof(res) + 4) == api.E_INVALID and b"aligned" in err()
        assert call(n=0) == api.E_INVALID and b"ctx is NULL" in err()
    else:
        assert call(n=0) == 0 and call(spans=0) == 0
        assert out[:19].tobytes() == lz4_ref.EMPTY and res.as_dict() == lz4_ref.encode(b"")[1]
        out[:19] = 0xAB
    assert (out == 0xAB).all()
    assert hip_lib.cfhip_lz4_encode_stage_ms(None, (ctypes.c_float*9)(), 9) == api.E_INVALID


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_decode_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    z = np.frombuffer(lz4_ref.twin(np.arange(5000, dtype=np.uint8)), np.uint8).copy()
    out = np.full(5000 + 8, 0xAB, np.uint8)
    res = api.Lz4DecodeResult()

    def call(z_ptr=z.ctypes.data, zbytes=z.size, out_ptr=out.ctypes.data, n=5000, res_ptr=ctypes.addressof(res)):
        if device:
            return hip_lib.cfhip_lz4_decode_device(None, z_ptr, zbytes, out_ptr, n, res_ptr, None)
        return hip_lib.cfhip_lz4_decode(None, z_ptr, zbytes, out_ptr, n, res_ptr)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(z_ptr=None) == api.E_INVALID and b"frame is NULL" in err()
    assert call(res_ptr=None) == api.E_INVALID and b"result is NULL" in err()
    assert call(out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(n=1 << 31) == api.E_CAPACITY and b"2^31" in err()
    assert call(zbytes=(1 << 32) + 1) == api.E_CAPACITY
    if device:
        assert call(out_ptr=out.ctypes.data + 2) == api.E_INVALID and b"aligned" in err()
        assert call(res_ptr=ctypes.addressof(res) + 4) == api.E_INVALID and b"aligned" in err()
        assert call(n=0, out_ptr=None) == api.E_INVALID and b"ctx is NULL" in err()
    assert (out == 0xAB).all()
    assert hip_lib.cfhip_lz4_decode_stage_ms(None, (ctypes.c_float*3)(), 3) == api.E_INVALID


def test_empty_frames_need_no_context(hip_lib):
    from cuttlefish_amd import api
    res = api.Lz4DecodeResult()

    def call(frame):
        z = np.frombuffer(frame, np.uint8)
        rc = hip_lib.cfhip_lz4_decode(None, z.ctypes.data, z.size, None, 0, ctypes.addressof(res))
        return rc, res.as_dict()
    desc = bytes([0x64, 0x40])                                 # no content size, a content checksum
    other = lz4_ref.MAGIC + desc + bytes([(lz4_ref.xxh32(desc) >> 8) & 0xFF]) + bytes(4) + b"\x05\x5D\xCC\x02"
    for frame in (lz4_ref.EMPTY, other):
        rc, r = call(frame)
        assert rc == 0 and r == lz4_ref.decode(frame, 0)[1] and r["bytes_in"] == len(frame)
    assert r["content_checksum"] == 1
    # and the same routines reject what the twin rejects
    for frame in (lz4_ref.EMPTY + b"\x00", lz4_ref.EMPTY[:-1], lz4_ref.EMPTY[:-1] + b"\x02", b"\x05" + lz4_ref.EMPTY[1:],
                  lz4_ref.twin(np.arange(5, dtype=np.uint8)), b"\x04\x22", other[:-1]):
        rc, r = call(frame)
        want = lz4_ref.decode(frame, 0)[1]
        assert rc == api.E_DATA and r == want and r["status"], frame
        text = hip_lib.cfhip_last_error(None).decode()
        assert lz4_ref.CLASSES[r["status"]] in text and "block %d" % r["bad_block"] in text


def test_python_surface():
    from cuttlefish_amd import Texture, api
    for f in (api.lz4_bound, api.Context.lz4_encode, api.Context.lz4_encode_device, api.Context.lz4_encode_result,
              api.Context.lz4_encode_stage_ms, api.Context.lz4_decode, api.Context.lz4_decode_device,
              api.Context.lz4_decode_result, api.Context.lz4_decode_stage_ms, Texture.pack, Texture.unpack):
        assert callable(f)
    t = Texture(8, 8)
    assert t.pack(codec="lz4") is None and t.pack() is None and Texture.unpack(t, lz4_ref.EMPTY) is None
    with pytest.raises(ValueError):
        t.pack(indexed=True, codec="lz4")
    with pytest.raises(ValueError):
        t.pack(codec="zstd")
    e = api.CfhipError(api.E_DATA, "lz4_decode: offset error in block 3", 6, 3)
    assert (e.code, e.status, e.bad_block) == (api.E_DATA, 6, 3)
