"""The inputs the LZ4 frame codec is tested on (tests/test_lz4_ref.py and tests/test_lz4_host.py on the CPU,
tests/test_gpu_lz4.py on the GPU), each built once per process together with the twin's result:

  * CASES: the contents zeros, text, odd, random, BC1, BC7, BC1 rdo of tests/deflate_cases.py at the sizes 0, 1, 4, 5,
    12, 13 (the first size that can hold a match), 4095, 4096, 4097 (the chunk end), 65535, 65536, 65537 (the block end,
    a last block of one byte) and 200 KiB, as far as each content reaches;
  * FOREIGN: liblz4's own frames of tests/golden/lz4_foreign.npz (tests/golden/make_lz4_foreign.py): set `a` without block
    checksums and content size but with a content checksum, set `b` the other way round, and the two rejected kinds;
  * MUTATIONS of two of the twin's frames and two foreign ones: bytes inverted in the header, the first size word and the
    frame's end, seeded single-bit flips, byte flips inside block bodies with the block checksum sealed again (so that
    tokens, lengths and offsets are reached behind a checksum), every size word +1, -1, its raw bit flipped, 0 and
    65537, truncations and appended bytes, headers changed with HC sealed again (linked, larger blocks, a dictionary id,
    version, reserved bits, content size), and out_bytes +- 1."""
import functools
import os
import struct

import numpy as np

import deflate_cases as C
import lz4_ref as R

SIZES = (0, 1, 4, 5, 12, 13, 4095, 4096, 4097, 65535, 65536, 65537, 200*1024)
CONTENTS = ("zeros", "text", "odd", "random", "BC1", "BC7", "BC1 rdo")
_OWN = {"BC1": 32768, "BC7": 65536, "BC1 rdo": 32768}
CASES = [(c, n) for c in CONTENTS for n in sorted(set(s for s in SIZES if s <= _OWN.get(c, C.BIG)) | {_OWN.get(c, C.BIG)})]
IDS = ["%s-%d" % (c.replace(" ", "_"), n) for c, n in CASES]

FOREIGN = (("text", 20000), ("BC1 rdo", 32768), ("BC7", 65537), ("zeros", 200*1024), ("random", 65537))
FOREIGN_IDS = ["%s-%s-%d" % (s, c.replace(" ", "_"), n) for s in "ab" for c, n in FOREIGN]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def content(name, n):
    a = C.content(name)
    return np.resize(a, n) if a.size < n else a[:n]       # BC7's payload is 65536 bytes: repeated to 65537


@functools.lru_cache(maxsize=None)
def twin(name, n):
    """-> (the frame, the result) of lz4_ref on a case, computed once per process"""
    return R.encode(content(name, n))


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "lz4_foreign.npz")) as f:
        return {k: f[k].tobytes() for k in f.files}


def foreign(which, i):
    """-> (the input bytes, liblz4's frame) of FOREIGN[i] in set `which` ('a' or 'b')"""
    name, n = FOREIGN[i]
    return content(name, n).tobytes(), fixture()["%s%d" % (which, i)]


FOREIGN_ALL = [(w, i) for w in "ab" for i in range(len(FOREIGN))]


def blocks_of(z: bytes):
    """-> [(position of the size word, size, raw)] of a well-formed frame, and whether blocks carry checksums"""
    flg = z[4]
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    bsum = (flg >> 4) & 1
    out = []
    while True:
        word = struct.unpack_from("<I", z, pos)[0]
        if not word:
            return out, bsum
        out.append((pos, word & 0x7FFFFFFF, word >> 31))
        pos += 4 + (word & 0x7FFFFFFF) + 4*bsum


def seal_header(z: bytes, desc: bytes) -> bytes:
    """z with its frame descriptor (FLG .. in front of HC) replaced and HC computed again"""
    flg = z[4]
    hlen = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    return z[:4] + desc + bytes([(R.xxh32(desc) >> 8) & 0xFF]) + z[hlen:]


def _mutate(tag, z, n, seed):
    """-> [(label, frame, out_bytes)]"""
    out = []

    def flip(at, mask):
        b = bytearray(z)
        b[at] ^= mask
        return bytes(b)
    for at in list(range(19)) + list(range(len(z) - 12, len(z))):
        out.append(("%s byte %d" % (tag, at), flip(at, 0xFF), n))
    rng = np.random.default_rng(seed)
    for bit in rng.integers(0, 8*len(z), 150):
        out.append(("%s bit %d" % (tag, bit), flip(int(bit) >> 3, 1 << (int(bit) & 7)), n))
    blocks, bsum = blocks_of(z)
    if bsum:
        for k in range(60):
            pos, size, raw = blocks[int(rng.integers(0, len(blocks)))]
            # the front of a block holds the densest tokens; half of the flips go there
            at = pos + 4 + int(rng.integers(0, min(size, 64) if k % 2 else size))
            b = bytearray(flip(at, 1 << int(rng.integers(0, 8))))
            b[pos + 4 + size:pos + 8 + size] = struct.pack("<I", R.xxh32(bytes(b[pos + 4:pos + 4 + size])))
            out.append(("%s sealed %d" % (tag, at), bytes(b), n))
    for i, (pos, size, raw) in enumerate(blocks):
        word = struct.unpack_from("<I", z, pos)[0]
        for what, w in (("+1", word + 1), ("-1", word - 1), ("raw", word ^ 0x80000000), ("0", 0), ("65537", 65537)):
            out.append(("%s block %d word %s" % (tag, i, what), z[:pos] + struct.pack("<I", w & 0xFFFFFFFF) + z[pos + 4:], n))
    for cut in (1, 4, 5, len(z)//2):
        out.append(("%s cut %d" % (tag, cut), z[:-cut], n))
    out.append((tag + " appended", z + b"\x00", n))
    out.append((tag + " appended end mark", z + b"\x00\x00\x00\x00", n))
    flg, bd = z[4], z[5]
    rest = z[6:14] if flg & 8 else b""
    for what, desc in (("linked", bytes([flg ^ 0x20, bd]) + rest), ("256K", bytes([flg, 0x50]) + rest),
                       ("1M", bytes([flg, 0x60]) + rest), ("4M", bytes([flg, 0x70]) + rest),
                       ("dict id", bytes([flg | 1, bd]) + rest + b"\x01\x00\x00\x00"),
                       ("version", bytes([(flg & 0x3F) | 0x80, bd]) + rest), ("reserved", bytes([flg | 2, bd]) + rest),
                       ("BD low", bytes([flg, bd | 1]) + rest), ("BD 3", bytes([flg, 0x30]) + rest)):
        out.append(("%s header %s" % (tag, what), seal_header(z, desc), n))
    if flg & 8:
        for d in (1, -1):
            out.append(("%s content size %+d" % (tag, d), seal_header(z, bytes([flg, bd]) + struct.pack("<Q", n + d)), n))
    else:
        out.append((tag + " content size added", seal_header(z, bytes([flg | 8, bd]) + struct.pack("<Q", n + 1)), n))
    out.append((tag + " n - 1", z, n - 1))
    out.append((tag + " n + 1", z, n + 1))
    return out


MUTATED = (("text", 65537), ("BC1 rdo", 32768))
MUTATED_FOREIGN = (("a", 2), ("b", 0))


@functools.lru_cache(maxsize=None)
def originals():
    """-> [(label, frame, out_bytes)] the mutations start from"""
    out = [("%s-%d" % (name, n), twin(name, n)[0], n) for name, n in MUTATED]
    for w, i in MUTATED_FOREIGN:
        out.append(("foreign-%s%d" % (w, i), foreign(w, i)[1], FOREIGN[i][1]))
    return out


@functools.lru_cache(maxsize=None)
def mutations():
    out = []
    for seed, (tag, z, n) in enumerate(originals()):
        out += _mutate(tag, z, n, 200 + seed)
    return out


@functools.lru_cache(maxsize=None)
def verdicts():
    """the twin on every mutation -> [(bytes or None, result)]"""
    return [R.decode(z, n) for _, z, n in mutations()]


@functools.lru_cache(maxsize=None)
def recorded_verdicts():
    """[(label, status, bad_block)] per mutation as recorded in tests/golden/lz4_mutations.json: what verdicts() gives,
    kept so that the GPU test need not run the twin on every record (tests/test_lz4_ref.py holds the file to it)"""
    import json
    with open(os.path.join(GOLDEN, "lz4_mutations.json")) as f:
        return [tuple(r) for r in json.load(f)]


def write_corpus(path, records):
    """records of (frame, out_bytes) in the format tools/lz4_host.cpp reads"""
    with open(path, "wb") as f:
        for z, n in records:
            f.write(struct.pack("<QQ", len(z), n))
            f.write(z)
