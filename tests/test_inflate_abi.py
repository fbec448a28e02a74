"""cfhip_inflate*, cfhip_deflate_indexed* and cfhip_zindex_entries without a GPU: the exports, the structs against the
header's text, the constants shared with the twin, the argument errors, every one of which returns before any device
call (a NULL context is reported last), the empty streams, which need no context, and the Python surface."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import deflate_ref
import inflate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_zindex_entries", "cfhip_deflate_indexed", "cfhip_deflate_indexed_device", "cfhip_inflate",
         "cfhip_inflate_device", "cfhip_inflate_stage_ms")


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
    R = api.InflateResult
    assert ctypes.sizeof(R) == 56
    assert tuple(n for n, _ in R._fields_) == inflate_ref.FIELDS
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert _struct_fields("cfhip_inflate_result") == [("uint64_t", n) for n in inflate_ref.FIELDS[:5]] + \
        [("uint32_t", n) for n in inflate_ref.FIELDS[5:]]
    E = api.ZIndexEntry
    assert ctypes.sizeof(E) == 16 and [getattr(E, n).offset for n, _ in E._fields_] == [0, 8]
    assert _struct_fields("cfhip_zindex_entry") == [("uint64_t", "header_bit"), ("uint64_t", "token_bit")]
    assert api.INFLATE_STAGES == ("decode", "resolve", "pack", "fold")
    assert api.INFLATE_CLASSES == inflate_ref.CLASSES and api.ZINDEX_CHUNK == inflate_ref.CHUNK


def test_constants_have_their_twins():
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    assert re.search(r"CFHIP_E_DATA = -6\b", header) and re.search(r"#define CFHIP_ABI_VERSION 1\b", header)
    from cuttlefish_amd import api
    assert api.E_DATA == -6
    names = ("OK", "WRAPPER", "INDEX", "HEADER", "CODE", "DISTANCE", "OVERRUN", "CHECKSUM")
    twin = (inflate_ref.OK, inflate_ref.E_WRAPPER, inflate_ref.E_INDEX, inflate_ref.E_HEADER, inflate_ref.E_CODE,
            inflate_ref.E_DISTANCE, inflate_ref.E_OVERRUN, inflate_ref.E_CHECKSUM)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "inflate.h")).read()
    for name, value in zip(names, twin):
        assert int(re.search(r"CFHIP_INFLATE_%s = (\d+)" % name, header).group(1)) == value
        macro = "CFINF_OK" if name == "OK" else "CFINF_E_" + name
        assert int(re.search(r"#define %s (\d+)u" % macro, shared).group(1)) == value
    assert int(re.search(r"#define CFINF_CHUNK (\d+)u", shared).group(1)) == inflate_ref.CHUNK
    assert int(re.search(r"#define CFINF_STAGES (\d+)", shared).group(1)) == 4


def test_zindex_entries(hip_lib):
    from cuttlefish_amd import api
    for n in (0, 1, 4095, 4096, 4097, 65536, 200*1024, (1 << 31) - 1, 1 << 40):
        assert api.zindex_entries(n) == inflate_ref.zindex_entries(n) == (n + 4095)//4096


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_deflate_indexed_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    data = np.arange(5000, dtype=np.uint8)
    out = np.full(api.deflate_bound(5000) + 8, 0xAB, np.uint8)
    index = np.full((3, 2), 0xABABABABABABABAB, np.uint64)
    res = api.DeflateResult()

    def call(n=5000, out_ptr=out.ctypes.data, cap=out.size, idx=index.ctypes.data, entries=2, res_ptr=ctypes.addressof(res)):
        span = (api.LzSpan*1)()
        span[0].bytes, span[0].n = data.ctypes.data, n
        if device:
            return hip_lib.cfhip_deflate_indexed_device(None, span, 1, out_ptr, cap, idx, entries, res_ptr, None)
        return hip_lib.cfhip_deflate_indexed(None, span, 1, out_ptr, cap, idx, entries, res_ptr)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(res_ptr=None) == api.E_INVALID and b"result is NULL" in err()
    assert call(idx=None) == api.E_INVALID and b"index is NULL" in err()
    assert call(entries=1) == api.E_CAPACITY and b"cfhip_zindex_entries" in err()
    assert call(cap=api.deflate_bound(5000) - 1) == api.E_CAPACITY and b"cfhip_deflate_bound" in err()
    assert call(n=4096, entries=1) == api.E_INVALID and b"ctx is NULL" in err()
    if device:
        assert call(idx=index.ctypes.data + 4) == api.E_INVALID and b"aligned" in err()
        assert call(n=0, entries=0, idx=None) == api.E_INVALID and b"ctx is NULL" in err()
    else:
        assert call(n=0, entries=0, idx=None) == 0
        assert out[:11].tobytes() == deflate_ref.EMPTY and res.as_dict() == deflate_ref.deflate(b"")[1]
        out[:11] = 0xAB
    assert (out == 0xAB).all() and (index == 0xABABABABABABABAB).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_inflate_argument_errors(hip_lib, device):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    z = np.frombuffer(deflate_ref.twin(np.arange(5000, dtype=np.uint8)), np.uint8).copy()
    index = np.zeros((2, 2), np.uint64)
    out = np.full(5000 + 8, 0xAB, np.uint8)
    res = api.InflateResult()

    def call(z_ptr=z.ctypes.data, zbytes=z.size, idx=index.ctypes.data, entries=2, out_ptr=out.ctypes.data, n=5000,
             res_ptr=ctypes.addressof(res)):
        if device:
            return hip_lib.cfhip_inflate_device(None, z_ptr, zbytes, idx, entries, out_ptr, n, res_ptr, None)
        return hip_lib.cfhip_inflate(None, z_ptr, zbytes, idx, entries, out_ptr, n, res_ptr)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(z_ptr=None) == api.E_INVALID and b"zstream is NULL" in err()
    assert call(res_ptr=None) == api.E_INVALID and b"result is NULL" in err()
    assert call(out_ptr=None) == api.E_INVALID and b"out is NULL" in err()
    assert call(idx=None) == api.E_INVALID and b"index is NULL" in err()
    assert call(entries=1) == api.E_CAPACITY and b"cfhip_zindex_entries" in err()
    assert call(n=1 << 31, entries=1 << 19) == api.E_CAPACITY and b"2^31" in err()
    assert call(zbytes=(1 << 32) + 1) == api.E_CAPACITY
    if device:
        assert call(out_ptr=out.ctypes.data + 2) == api.E_INVALID and b"aligned" in err()
        assert call(idx=index.ctypes.data + 4) == api.E_INVALID and b"aligned" in err()
        assert call(n=0, entries=0, idx=None, out_ptr=None) == api.E_INVALID and b"ctx is NULL" in err()
    assert (out == 0xAB).all()
    assert hip_lib.cfhip_inflate_stage_ms(None, (ctypes.c_float*4)()) == api.E_INVALID


def test_empty_streams_need_no_context(hip_lib):
    from cuttlefish_amd import api
    res = api.InflateResult()

    def call(stream):
        z = np.frombuffer(stream, np.uint8)
        rc = hip_lib.cfhip_inflate(None, z.ctypes.data, z.size, None, 0, None, 0, ctypes.addressof(res))
        return rc, res.as_dict()
    for stream in (deflate_ref.EMPTY, zlib.compress(b"")):
        rc, r = call(stream)
        want = dict(inflate_ref.inflate_indexed(stream, [], 0)[1], rounds=0)
        assert rc == 0 and r == want and r["adler32"] == 1 and r["bytes_in"] == len(stream)
    # and the same routine rejects what the twin rejects
    for stream in (deflate_ref.EMPTY + b"\x00", deflate_ref.EMPTY[:-1], deflate_ref.EMPTY[:-1] + b"\x02",
                   b"\x79" + deflate_ref.EMPTY[1:], deflate_ref.twin(np.arange(5, dtype=np.uint8)), b"\x78"):
        rc, r = call(stream)
        want = inflate_ref.inflate_indexed(stream, [], 0)[1]
        assert rc == api.E_DATA and (r["status"], r["bad_chunk"]) == (want["status"], want["bad_chunk"]) and r["status"]
        text = hip_lib.cfhip_last_error(None).decode()
        assert inflate_ref.CLASSES[r["status"]] in text and "chunk 0" in text


def test_python_surface():
    from cuttlefish_amd import Texture, api
    for f in (api.Context.deflate_indexed, api.Context.deflate_indexed_device, api.Context.inflate,
              api.Context.inflate_result, api.Context.inflate_device, api.Context.inflate_stage_ms, api.zindex_entries,
              Texture.pack, Texture.unpack):
        assert callable(f)
    t = Texture(8, 8)
    assert t.pack(indexed=True) is None and t.pack() is None
    assert Texture.unpack(t, deflate_ref.EMPTY, []) is None
    e = api.CfhipError(api.E_DATA, "inflate: code error in chunk 3", 4, 3)
    assert (e.code, e.status, e.bad_chunk) == (api.E_DATA, 4, 3)
