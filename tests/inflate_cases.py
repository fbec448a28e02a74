"""The inputs the indexed inflater is tested on (tests/test_inflate_ref.py and tests/test_inflate_host.py on the CPU,
tests/test_gpu_inflate.py on the GPU), each built once per process together with the twin's verdict on it:

  * the encoder's own streams: tests/deflate_cases.py, by import;
  * FOREIGN streams: zlib.compressobj flushed with Z_SYNC_FLUSH after every 4096 input bytes -- an independent
    encoder's blocks and block-type choices, empty stored blocks between the chunks, a final block with no output --
    at levels 0, 1, 6, 9 and with Z_FIXED, Z_RLE and Z_HUFFMAN_ONLY, on text, zeros, BC7 and random at 20000 and 65537;
  * MUTATIONS of text-65537, BC1-32768 and one foreign stream: each byte of the first 64 and the last 8 inverted, 200
    seeded single-bit flips, a byte appended, the last byte removed, an entry's token_bit and header_bit +- 1, two entries
    swapped, n +- 1.

What the counters of a passing stream are.  cfhip_inflate_result counts the tokens READ.  For a group the encoder wrote
with Huffman codes those are the parse's tokens, deflate_ref's counts; a STORED group holds no tokens, every byte of it
is read as a literal, whatever the parse found there (random-204800: the parse finds two matches of four bytes, and all
four groups are stored).  counts_read() is deflate_ref's result with the stored groups counted that way."""
import functools
import struct
import zlib

import numpy as np

import deflate_cases as C
import deflate_ref as D
import inflate_ref as I
import lzsize_ref as Z

FOREIGN_MODES = (("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("level1", 1, zlib.Z_DEFAULT_STRATEGY),
                 ("level6", 6, zlib.Z_DEFAULT_STRATEGY), ("level9", 9, zlib.Z_DEFAULT_STRATEGY),
                 ("fixed", 6, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE), ("huffman", 6, zlib.Z_HUFFMAN_ONLY))
FOREIGN = [(content, n, mode) for content in ("text", "zeros", "BC7", "random") for n in (20000, 65537)
           for mode in range(len(FOREIGN_MODES))]
FOREIGN_IDS = ["%s-%d-%s" % (c, n, FOREIGN_MODES[m][0]) for c, n, m in FOREIGN]


def _content(name, n):
    a = C.content(name)
    return np.resize(a, n) if a.size < n else a[:n]       # BC7's payload is 65536 bytes: repeated to 65537


def flushed(x: bytes, level, strategy) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    out = b""
    for s in range(0, len(x), I.CHUNK):
        out += co.compress(x[s:s + I.CHUNK]) + co.flush(zlib.Z_SYNC_FLUSH)
    return out + co.flush()


@functools.lru_cache(maxsize=None)
def foreign(content, n, mode):
    """-> (the input bytes, the flushed zlib stream, its index)"""
    x = _content(content, n).tobytes()
    z = flushed(x, *FOREIGN_MODES[mode][1:])
    return x, z, I.build_index(z)


@functools.lru_cache(maxsize=None)
def own_index(name, n):
    return I.build_index(C.twin(name, n)[0])


@functools.lru_cache(maxsize=None)
def own_verdict(name, n):
    """-> the twin's (bytes, result) on a case's own stream and index, once per process"""
    return I.inflate_indexed(C.twin(name, n)[0], own_index(name, n), n)


@functools.lru_cache(maxsize=None)
def foreign_verdict(content, n, mode):
    x, z, index = foreign(content, n, mode)
    return I.inflate_indexed(z, index, len(x))


@functools.lru_cache(maxsize=None)
def counts_read(name, n):
    """-> deflate_ref's literals, matches, matched_bytes and adler32 of a case, its stored groups read as literals"""
    _, res = C.twin(name, n)
    keys = ("literals", "matches", "matched_bytes", "adler32")
    if not res["blocks_stored"]:
        return {k: res[k] for k in keys}
    if not res["blocks_fixed"] + res["blocks_dynamic"]:
        return dict(literals=n, matches=0, matched_bytes=0, adler32=res["adler32"])
    a = C.data(name, n)
    lits, (mp, ml, md) = Z.parse(a)
    out = dict(literals=0, matches=0, matched_bytes=0, adler32=res["adler32"])
    groups = (n + Z.COSTBLK - 1)//Z.COSTBLK
    for g in range(groups):
        lo, hi = g*Z.COSTBLK, min(n, (g + 1)*Z.COSTBLK)
        mi = (mp >= lo) & (mp < hi)
        gl = lits[(lits >= lo) & (lits < hi)]
        _, form = D._group(a, lo, hi, gl, (mp[mi], ml[mi], md[mi]), g == groups - 1)
        if form == 0:
            out["literals"] += hi - lo
        else:
            out["literals"] += int(gl.size)
            out["matches"] += int(mi.sum())
            out["matched_bytes"] += int(ml[mi].sum())
    return out


def _mutate(tag, z, index, n, seed):
    """-> [(label, stream, index, n)]"""
    out = []
    idx = [tuple(e) for e in index]

    def flip(at, mask):
        b = bytearray(z)
        b[at] ^= mask
        return bytes(b)
    for at in list(range(64)) + list(range(len(z) - 8, len(z))):
        out.append(("%s byte %d" % (tag, at), flip(at, 0xFF), idx, n))
    rng = np.random.default_rng(seed)
    for bit in rng.integers(0, 8*len(z), 200):
        out.append(("%s bit %d" % (tag, bit), flip(int(bit) >> 3, 1 << (int(bit) & 7)), idx, n))
    out.append((tag + " appended", z + b"\x00", idx, n))
    out.append((tag + " removed", z[:-1], idx, n))
    k = len(idx)//2
    for which in (0, 1):
        for d in (1, -1):
            e = list(idx[k])
            e[which] += d
            out.append(("%s entry %d[%d] %+d" % (tag, k, which, d), z, idx[:k] + [tuple(e)] + idx[k + 1:], n))
    out.append((tag + " entries swapped", z, [idx[0], idx[2], idx[1]] + idx[3:], n))
    out.append((tag + " n - 1", z, idx, n - 1))
    out.append((tag + " n + 1", z, idx + [(0, 0)], n + 1))
    return out


MUTATED = (("text", 65537), ("BC1", 32768))
MUTATED_FOREIGN = ("text", 20000, 2)


@functools.lru_cache(maxsize=None)
def originals():
    """-> [(label, stream, index, n, the bytes)] the mutations start from"""
    out = []
    for name, n in MUTATED:
        out.append(("%s-%d" % (name, n), C.twin(name, n)[0], own_index(name, n), n, C.data(name, n).tobytes()))
    x, z, index = foreign(*MUTATED_FOREIGN)
    out.append(("foreign", z, index, len(x), x))
    return out


@functools.lru_cache(maxsize=None)
def mutations():
    out = []
    for seed, (tag, z, index, n, _) in enumerate(originals()):
        out += _mutate(tag, z, index, n, 100 + seed)
    return out


@functools.lru_cache(maxsize=None)
def verdicts():
    """the twin on every mutation -> [(bytes or None, result)]; anything but a verdict propagates"""
    return [I.inflate_indexed(z, index, n) for _, z, index, n in mutations()]


@functools.lru_cache(maxsize=None)
def recorded_verdicts():
    """[(label, status, bad_chunk)] per mutation as recorded in tests/golden/inflate_mutations.json: what verdicts()
    gives, kept so that the GPU test need not run the twin 843 times (tests/test_inflate_ref.py holds the file to it)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_mutations.json")) as f:
        return [tuple(r) for r in json.load(f)]


def write_corpus(path, records):
    """records of (stream, index, n) in the format tools/inflate_host.cpp reads"""
    with open(path, "wb") as f:
        for z, index, n in records:
            f.write(struct.pack("<QQQ", len(z), n, len(index)))
            f.write(z)
            for hb, tb in index:
                f.write(struct.pack("<QQ", hb & (2**64 - 1), tb & (2**64 - 1)))


def index_array(index):
    """-> the index as the (entries, 2) uint64 array Context.inflate takes"""
    return np.array([[hb & (2**64 - 1), tb & (2**64 - 1)] for hb, tb in index], np.uint64).reshape(-1, 2)
