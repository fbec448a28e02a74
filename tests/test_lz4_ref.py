"""The LZ4 twin, tests/lz4_ref.py, on the CPU: its XXH32 against the xxhash module, its decoder against its encoder,
the merging and the rules of a block's end, the header and the bound, the recorded verdicts of the mutation corpus, a
size guard against liblz4 -- and, where ctypes finds liblz4.so.1, both directions against the library itself: it reads
every frame the twin writes, and the twin reads its frames (made here, and those of tests/golden/lz4_foreign.npz)."""
import ctypes
import struct

import numpy as np
import pytest

import deflate_cases as C
import lz4_cases as LC
import lz4_ref as R
import lzsize_ref as Z

REF_CASES = C.CASES + [("text", 12), ("text", 13), ("zeros", 12), ("zeros", 13)]
REF_IDS = C.IDS + ["text-12", "text-13", "zeros-12", "zeros-13"]


def _liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    lib.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    lib.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.LZ4F_decompress.restype = ctypes.c_size_t
    lib.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lib.LZ4F_isError.argtypes = [ctypes.c_size_t]
    lib.LZ4_compress_default.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_compressBound.argtypes = [ctypes.c_int]
    return lib


LIB = _liblz4()
needs_lib = pytest.mark.skipif(LIB is None, reason="liblz4.so.1 is absent")


def lz4f_decompress(z: bytes, n: int) -> bytes:
    ctx = ctypes.c_void_p()
    assert not LIB.LZ4F_isError(LIB.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    try:
        out = ctypes.create_string_buffer(n + 1)                # one byte more: a frame that holds more shows
        dn, sn = ctypes.c_size_t(n + 1), ctypes.c_size_t(len(z))
        r = LIB.LZ4F_decompress(ctx, out, ctypes.byref(dn), z, ctypes.byref(sn), None)
        assert not LIB.LZ4F_isError(r) and r == 0, r            # 0: the frame is complete
        assert sn.value == len(z) and dn.value == n
        return out.raw[:n]
    finally:
        LIB.LZ4F_freeDecompressionContext(ctx)


def test_xxh32_against_xxhash():
    import xxhash
    assert R.xxh32(b"", 0) == 0x02CC5D05
    rng = np.random.default_rng(3)
    for n in list(range(101)) + [65536]:
        d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        assert R.xxh32(d) == xxhash.xxh32(d).intdigest(), n
    assert R.xxh32(b"abc", 7) == xxhash.xxh32(b"abc", seed=7).intdigest()


def test_bound_and_header_bytes():
    for n in (0, 1, 65535, 65536, 65537, 200*1024, (1 << 31) - 1):
        assert R.lz4_bound(n) == 19 + n + 8*((n + 65535)//65536)
    h = R.header(70000)
    assert len(h) == R.HEADER_BYTES == 15 and h[:4] == b"\x04\x22\x4D\x18" and h[4] == 0x78 and h[5] == 0x40
    assert struct.unpack_from("<Q", h, 6)[0] == 70000 and h[14] == (R.xxh32(h[4:14]) >> 8) & 0xFF
    assert R.EMPTY == R.header(0) + bytes(4) and len(R.EMPTY) == 19 == R.lz4_bound(0)
    assert R.encode(b"") == (R.EMPTY, dict.fromkeys(R.FIELDS, 0) | {"bytes_out": 19})
    assert R.decode(R.EMPTY, 0)[0] == b""


@pytest.mark.parametrize("name,n", REF_CASES, ids=REF_IDS)
def test_decoder_inverts_encoder(name, n):
    a = C.data(name, n)
    frame, res = R.encode(a)
    assert len(frame) == res["bytes_out"] <= R.lz4_bound(n) and res["bytes_in"] == n
    assert res["blocks_compressed"] + res["blocks_stored"] == (n + R.BLOCK - 1)//R.BLOCK
    out, dres = R.decode(frame, n)
    assert out == a.tobytes() and dres["status"] == 0 and dres["bytes_out"] == n
    assert all(dres[k] == res[k] for k in R.FIELDS[2:])
    if LIB is not None:
        assert lz4f_decompress(frame, n) == a.tobytes()


def test_merging_makes_zeros_one_sequence():
    a = np.zeros(65536, np.uint8)
    assert R.block_matches(a) == [(1, 65536 - 5 - 1, 1)]
    frame, res = R.encode(a)
    assert (res["sequences"], res["literals"], res["matched_bytes"]) == (2, 6, 65530) and res["blocks_compressed"] == 1
    # across a chunk end, and not across a literal or a change of distance
    raw = Z.parse(a)[1]
    assert len(raw[0]) > 16 and set(raw[2].tolist()) == {1}
    b = np.concatenate([np.zeros(5000, np.uint8), np.arange(1, 9, dtype=np.uint8), np.zeros(5000, np.uint8)])
    m = R.block_matches(b)
    assert m[0] == (1, 4999, 1) and all(p >= 5008 for p, _, _ in m[1:]) and len(m) <= 3


def test_end_rules_on_hand_built_inputs():
    # a repeat that would run to the block's end: cut five bytes before it
    pat = np.frombuffer(b"abcdefgh", np.uint8)
    for n in (13, 14, 16, 17, 20, 21, 24, 40, 4100, 65536):
        a = np.resize(pat, n)
        for p, l, d in R.block_matches(a):
            assert p <= n - 12 and p + l <= n - 5 and l >= 4, (n, p, l)
        frame, _ = R.encode(a)
        assert R.decode(frame, n)[0] == a.tobytes()
    assert R.block_matches(np.resize(pat, 20)) == [(8, 7, 8)]                 # starts at n - 12, ends at n - 5
    assert R.block_matches(np.resize(pat, 19)) == []                          # would start at n - 11
    # a match found late in the block becomes literals; one that would keep fewer than 4 bytes too
    rng = np.random.default_rng(5)
    head = rng.integers(0, 256, 64).astype(np.uint8)
    late = np.concatenate([head, rng.integers(0, 256, 40).astype(np.uint8), head[:10]])
    assert Z.parse(late)[1][0].tolist() == [104] and R.block_matches(late) == []      # 104 > 114 - 12
    short = np.concatenate([head, rng.integers(0, 256, 40).astype(np.uint8), head[:10], rng.integers(0, 256, 4).astype(np.uint8)])
    # 104 <= 118 - 12: it stays, cut from 10 bytes to the 9 that end at 118 - 5.  (A match that starts no later than
    # n - 12 keeps at least 7 bytes, so the format's "fewer than 4 left" rule is never the one that decides.)
    assert Z.parse(short)[1][0].tolist() == [104] and R.block_matches(short) == [(104, 9, 104)]
    for n in range(13):
        assert R.block_matches(np.zeros(n, np.uint8)) == []
    assert R.encode(np.zeros(12, np.uint8))[1]["blocks_stored"] == 1
    # 13 zeros, the first size that can hold a match: it starts at 1 = n - 12 and is cut to 7 bytes; 4 + 6 bytes < 13
    assert R.block_matches(np.zeros(13, np.uint8)) == [(1, 7, 1)]
    r = R.encode(np.zeros(13, np.uint8))[1]
    assert (r["blocks_compressed"], r["sequences"], r["literals"], r["matched_bytes"], r["bytes_out"]) == (1, 2, 6, 7, 19 + 8 + 10)


def test_random_is_stored_and_text_is_not():
    assert R.encode(C.data("random", 65537))[1]["blocks_stored"] == 2
    r = R.encode(C.data("text", 65537))[1]
    assert (r["blocks_compressed"], r["blocks_stored"]) == (1, 1)                  # a last block of one byte is stored


def test_decoder_classes_on_hand_built_frames():
    body = bytes([0x10, 0x41, 0x01, 0x00])                     # one literal, then offset 1 with nothing behind it

    def frame(blocks, n, flg=0x60, tail=b""):
        desc = bytes([flg, 0x40])
        z = R.MAGIC + desc + bytes([(R.xxh32(desc) >> 8) & 0xFF])
        for b in blocks:
            z += struct.pack("<I", len(b)) + b
        return z + bytes(4) + tail

    def verdict(z, n):
        r = R.decode(z, n)[1]
        return r["status"], r["bad_block"]
    lit = bytes([0x50]) + b"hello"
    assert R.decode(frame([lit], 5), 5)[0] == b"hello"
    assert verdict(frame([lit], 5), 6) == (R.E_SIZE, 0)
    assert verdict(frame([lit], 5), 4) == (R.E_SEQUENCE, 0)
    assert verdict(frame([bytes([0x10, 0x41, 0x00, 0x00, 0x00])], 6), 6) == (R.E_OFFSET, 0)
    assert verdict(frame([bytes([0x10, 0x41, 0x02, 0x00, 0x00])], 6), 6) == (R.E_OFFSET, 0)
    assert verdict(frame([bytes([0x10, 0x41, 0x01])], 6), 6) == (R.E_SEQUENCE, 0)
    assert verdict(frame([bytes([0xF0])], 6), 6) == (R.E_SEQUENCE, 0)
    assert verdict(frame([bytes([0x11, 0x41, 0x01, 0x00])], 5), 5) == (R.E_SEQUENCE, 0)      # the match leaves the output
    assert verdict(frame([bytes([0x11, 0x41, 0x01, 0x00])], 6), 6) == (R.E_SEQUENCE, 0)      # no last sequence
    assert R.decode(frame([bytes([0x11, 0x41, 0x01, 0x00, 0x00])], 6), 6)[0] == b"AAAAAA"
    assert verdict(frame([lit], 5, tail=b"\x00"), 5) == (R.E_BLOCKS, 1)
    assert verdict(frame([lit], 5)[:-1], 5) == (R.E_BLOCKS, 1)
    assert verdict(frame([], 5), 5) == (R.E_SIZE, 0)
    assert verdict(frame([lit], 5, flg=0x64), 5) == (R.E_BLOCKS, 1)                         # no room for the content checksum
    r = R.decode(frame([lit], 5, flg=0x64, tail=b"\x01\x02\x03\x04"), 5)
    assert r[0] == b"hello" and r[1]["content_checksum"] == 1                               # present, not verified
    assert verdict(frame([lit], 5, flg=0x40), 5) == (R.E_UNSUPPORTED, 0)
    assert verdict(b"\x04\x22\x4D", 5) == (R.E_HEADER, 0) and verdict(frame([body], 2)[:6], 2) == (R.E_HEADER, 0)


def test_recorded_mutation_verdicts_are_the_twins():
    got = [(label, res["status"], res["bad_block"]) for (label, _, _), (_, res) in zip(LC.mutations(), LC.verdicts())]
    assert got == LC.recorded_verdicts()


def test_fixture_frames_decode_and_the_rejected_kinds_are_unsupported():
    for w, i in LC.FOREIGN_ALL:
        x, z = LC.foreign(w, i)
        out, res = R.decode(z, len(x))
        assert out == x and res["status"] == 0 and res["content_checksum"] == (w == "a"), (w, i)
    for key in ("linked", "big"):
        res = R.decode(LC.fixture()[key], 200*1024)[1]
        assert (res["status"], res["bad_block"]) == (R.E_UNSUPPORTED, 0), key


@needs_lib
def test_liblz4_reads_gpu_case_frames_and_its_own_fresh_frames_decode():
    """the GPU suite's cases (tests/lz4_cases.py) through LZ4F_decompress, and frames made by the library now -- not the
    fixture's copies -- through the twin"""
    import importlib.util
    import os
    for name, n in LC.CASES:
        assert lz4f_decompress(LC.twin(name, n)[0], n) == LC.content(name, n).tobytes(), (name, n)
    spec = importlib.util.spec_from_file_location("make_lz4_foreign", os.path.join(LC.GOLDEN, "make_lz4_foreign.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    for i, (name, n) in enumerate(LC.FOREIGN):
        x = LC.content(name, n).tobytes()
        for kw, key in ((dict(content_checksum=1), "a%d" % i), (dict(content_size=1, block_checksum=1), "b%d" % i)):
            z = mk.compress_frame(LIB, x, **kw)             # (another version of the library may parse otherwise than
            assert z[:7] == LC.fixture()[key][:7]               # the fixture's: only the header's start is compared)
            assert R.decode(z, n)[0] == x
    zeros = bytes(200*1024)
    for kw in (dict(independent=0), dict(block_id=5)):
        assert R.decode(mk.compress_frame(LIB, zeros, **kw), len(zeros))[1]["status"] == R.E_UNSUPPORTED
        assert lz4f_decompress(mk.compress_frame(LIB, zeros, **kw), len(zeros)) == zeros


# The twin against LZ4_compress_default per independent 64 KiB block, as a fraction of the raw size.  Over the corpus of
# tools/bench_lz4.py --ratio (32 photographic payloads and their rdo_ref versions; profiles/lz4_ratio.md) the twin's
# frame was never larger than liblz4-default's: (twin - default) / raw ran from -0.0477 to -0.0021, so the worst excess
# measured is EXCESS_MEASURED of the raw size (negative: the twin is smaller everywhere).  The guard allows that plus
# 0.02.  On the two guarded inputs themselves the same file measures -0.0218 (BC1 rdo) and -0.1203 (text).
EXCESS_MEASURED = -0.0021
EXCESS_ALLOWED = EXCESS_MEASURED + 0.02


@needs_lib
@pytest.mark.parametrize("name,n", [("BC1 rdo", 32768), ("text", 200*1024)], ids=["BC1_rdo", "text"])
def test_size_guard_against_liblz4_default(name, n):
    a = LC.content(name, n).tobytes()
    ours = len(LC.twin(name, n)[0])
    theirs = 19
    for s in range(0, n, R.BLOCK):
        blk = a[s:s + R.BLOCK]
        cap = LIB.LZ4_compressBound(len(blk))
        out = ctypes.create_string_buffer(cap)
        c = LIB.LZ4_compress_default(blk, out, len(blk), cap)
        assert c > 0
        theirs += 8 + min(c, len(blk))
    print("%s-%d: twin %d (%.4f), liblz4 default %d (%.4f)" % (name, n, ours, ours/n, theirs, theirs/n))
    assert ours <= theirs + EXCESS_ALLOWED*n
