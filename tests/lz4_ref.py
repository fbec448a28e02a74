"""LZ4 frames of a byte stream in Python -- THE DEFINITION of every byte csrc/lz4.hip writes and of every verdict it
gives.  Every constant has its twin in csrc/lz4.h.

THE ENCODER.  The stream a[0..N), N < 2^31 (several spans: their concatenation), becomes one LZ4 frame (LZ4 Frame
Format 1.6):

  magic 04 22 4D 18; FLG 0x78 (version 01, independent blocks, block checksums, content size, no content checksum, no
  dictionary id); BD 0x40 (64 KiB blocks); N in 8 little-endian bytes; HC = (XXH32(FLG .. N, 0) >> 8) & 0xFF;
  per started 65536 input bytes one block: a little-endian size word (bit 31: stored raw), the bytes, the little-endian
  XXH32 (seed 0) of the bytes as stored; the end mark 00 00 00 00.  An empty input: the 15 header bytes and the end mark.

  * tokens: block b, TAKEN AS A STREAM OF ITS OWN, is parsed by lzsize_ref (matches and parse: K, MIN, MAX, CHUNK as they
    are, every candidate inside the block);
  * merging: a match that follows a match with no literal between them and has the same distance is added to it (across
    chunk ends too): a run of zeros is one sequence;
  * the end of the block, after merging, n the block's length: n < 13: all literals.  A match that starts after n - 12
    becomes literals; a match that ends after n - 5 is cut to end there, and becomes literals if fewer than 4 bytes stay;
  * sequences as the LZ4 block format has them: token (literal length << 4 | match length - 4, 15 = more follows), the
    255-runs, the literals, the offset in two little-endian bytes, the match length's 255-runs; the last sequence is
    literals only;
  * a block whose encoding is not smaller than its bytes is stored raw.

The result: bytes_in, bytes_out, blocks_compressed, blocks_stored, and over the COMPRESSED blocks sequences (the last,
literal-only one of each included), literals (bytes) and matched_bytes -- what a decoder can count again.

THE DECODER reads exactly one frame of `len(frame)` bytes into `out_bytes` bytes and answers with a class, in this order:

  header   fewer than 7 bytes or a wrong magic -> HEADER; version != 01, FLG bit 1, BD bits 7 and 3..0, a block-size code
           below 4 -> HEADER; the frame shorter than its header or a wrong HC -> HEADER; linked blocks, a dictionary id, a
           block-size code above 4 -> UNSUPPORTED; a content size other than out_bytes -> SIZE.  bad_block is 0.
  chain    blocks b = 0 .. ceil(out_bytes / 65536) - 1 in order.  The size word leaves the stream -> BLOCKS; the word is 0
           (the end mark, early) -> SIZE; a size above 65536 or a raw block of 0 bytes -> BLOCKS; the bytes or the checksum
           leave the stream -> BLOCKS.  Then block b itself (below).  After the last block: no room for the end mark, a word
           other than 0, no room for the content checksum (where FLG announces one; it is NOT verified), or bytes behind
           the frame -> BLOCKS at bad_block = the number of blocks.
  block    want = 65536, or what is left of out_bytes for the last.  The block checksum, where present -> CHECKSUM.  Raw:
           size != want -> SIZE.  Compressed, from ip = op = 0: no byte for the token or for a length byte -> SEQUENCE;
           literals that leave the input, then the output -> SEQUENCE; input used up: the block ends; fewer than two bytes
           for the offset -> SEQUENCE; offset 0 or above op -> OFFSET; a match that leaves the output -> SEQUENCE.  At
           the end op != want -> SIZE.

The first failing block in stream order gives (status, bad_block); the bytes are then undefined (None here)."""
import struct

import numpy as np

import lzsize_ref as Z

BLOCK = 65536                    # CFLZ4_BLOCK
MAGIC = b"\x04\x22\x4D\x18"
FLG, BD = 0x78, 0x40
HEADER_BYTES = 15
LAST_LITERALS = 5                # the last bytes of a block are literals           (CFLZ4_LAST_LITERALS)
MATCH_MARGIN = 12                # no match starts later than this before the end   (CFLZ4_MATCH_MARGIN)

FIELDS = ("bytes_in", "bytes_out", "blocks_compressed", "blocks_stored", "sequences", "literals", "matched_bytes")
DECODE_FIELDS = FIELDS + ("status", "bad_block", "content_checksum", "reserved")

OK, E_HEADER, E_UNSUPPORTED, E_BLOCKS, E_CHECKSUM, E_SEQUENCE, E_OFFSET, E_SIZE = range(8)
CLASSES = ("ok", "header", "unsupported", "blocks", "checksum", "sequence", "offset", "size")

P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data, seed=0) -> int:
    """XXH32 in plain Python"""
    data = bytes(data)
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32]
        while p + 16 <= n:
            for i, w in enumerate(struct.unpack_from("<4I", data, p)):
                v[i] = (_rotl((v[i] + w*P2) & M32, 13)*P1) & M32
            p += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, p)[0]*P3) & M32, 17)*P4) & M32
        p += 4
    while p < n:
        h = (_rotl((h + data[p]*P5) & M32, 11)*P1) & M32
        p += 1
    h ^= h >> 15
    h = (h*P2) & M32
    h ^= h >> 13
    h = (h*P3) & M32
    return h ^ (h >> 16)


def lz4_bound(n: int) -> int:
    return 19 + n + 8*((n + BLOCK - 1)//BLOCK)


def header(n: int) -> bytes:
    desc = bytes([FLG, BD]) + struct.pack("<Q", n)
    return MAGIC + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


EMPTY = header(0) + b"\x00\x00\x00\x00"


def block_matches(a: np.ndarray):
    """-> [(start, length, distance)] of one block after merging and the end rules"""
    n = a.size
    if n < MATCH_MARGIN + 1:
        return []
    _, (mp, ml, md) = Z.parse(a)
    merged = []
    for p, l, d in zip(mp.tolist(), ml.tolist(), md.tolist()):
        if merged and merged[-1][0] + merged[-1][1] == p and merged[-1][2] == d:
            merged[-1][1] += l
        else:
            merged.append([p, l, d])
    out = []
    for p, l, d in merged:
        if p > n - MATCH_MARGIN:
            continue
        if p + l > n - LAST_LITERALS:
            l = n - LAST_LITERALS - p
            if l < Z.MIN:
                continue
        out.append((p, l, d))
    return out


def _runs(v: int) -> bytes:
    """the bytes behind a nibble of 15: v - 15 in 255-runs"""
    v -= 15
    return b"\xFF"*(v//255) + bytes([v % 255])


def encode_block(a: np.ndarray):
    """-> (the LZ4 block of a, sequences, literal bytes, matched bytes)"""
    raw = a.tobytes()
    out, at, lits, matched = [], 0, 0, 0
    seqs = block_matches(a)
    for p, l, d in seqs:
        ll = p - at
        out.append(bytes([(min(ll, 15) << 4) | min(l - 4, 15)]))
        if ll >= 15:
            out.append(_runs(ll))
        out.append(raw[at:p])
        out.append(struct.pack("<H", d))
        if l - 4 >= 15:
            out.append(_runs(l - 4))
        at = p + l
        lits += ll
        matched += l
    ll = len(raw) - at
    out.append(bytes([min(ll, 15) << 4]))
    if ll >= 15:
        out.append(_runs(ll))
    out.append(raw[at:])
    return b"".join(out), len(seqs) + 1, lits + ll, matched


def encode(spans):
    """-> (the frame, the result) of the concatenation of the spans"""
    a = Z.stream(spans)
    n = a.size
    assert n < 1 << 31
    res = dict.fromkeys(FIELDS, 0)
    res["bytes_in"] = n
    out = [header(n)]
    for s in range(0, n, BLOCK):
        blk = a[s:s + BLOCK]
        enc, seqs, lits, matched = encode_block(blk)
        if len(enc) >= blk.size:
            body = blk.tobytes()
            out.append(struct.pack("<I", blk.size | 0x80000000))
            res["blocks_stored"] += 1
        else:
            body = enc
            out.append(struct.pack("<I", len(enc)))
            res["blocks_compressed"] += 1
            res["sequences"] += seqs
            res["literals"] += lits
            res["matched_bytes"] += matched
        out.append(body)
        out.append(struct.pack("<I", xxh32(body)))
    out.append(b"\x00\x00\x00\x00")
    frame = b"".join(out)
    res["bytes_out"] = len(frame)
    assert len(frame) <= lz4_bound(n)
    return frame, res


def twin(spans) -> bytes:
    return encode(spans)[0]


def parse_header(z: bytes, out_bytes: int):
    """-> (status, header length, block checksums, content checksum)"""
    if len(z) < 7 or z[:4] != MAGIC:
        return E_HEADER, 0, 0, 0
    flg, bd = z[4], z[5]
    if (flg >> 6) != 1 or (flg & 2) or (bd & 0x8F) or ((bd >> 4) & 7) < 4:
        return E_HEADER, 0, 0, 0
    hlen = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if len(z) < hlen or z[hlen - 1] != (xxh32(z[4:hlen - 1]) >> 8) & 0xFF:
        return E_HEADER, 0, 0, 0
    if not (flg & 0x20) or (flg & 1) or ((bd >> 4) & 7) != 4:
        return E_UNSUPPORTED, 0, 0, 0
    if (flg & 8) and struct.unpack_from("<Q", z, 6)[0] != out_bytes:
        return E_SIZE, 0, 0, 0
    return OK, hlen, (flg >> 4) & 1, (flg >> 2) & 1


def decode_block(src: bytes, want: int):
    """one compressed block -> (status, the bytes or None, sequences, literal bytes, matched bytes)"""
    size, ip = len(src), 0
    out = bytearray()
    seqs = lits = matched = 0
    while True:
        if ip >= size:
            return E_SEQUENCE, None, 0, 0, 0
        token = src[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            while True:
                if ip >= size:
                    return E_SEQUENCE, None, 0, 0, 0
                b = src[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        if ll > size - ip or ll > want - len(out):
            return E_SEQUENCE, None, 0, 0, 0
        out += src[ip:ip + ll]
        ip += ll
        seqs += 1
        lits += ll
        if ip == size:
            break
        if size - ip < 2:
            return E_SEQUENCE, None, 0, 0, 0
        off = src[ip] | (src[ip + 1] << 8)
        ip += 2
        if off == 0 or off > len(out):
            return E_OFFSET, None, 0, 0, 0
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= size:
                    return E_SEQUENCE, None, 0, 0, 0
                b = src[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if ml > want - len(out):
            return E_SEQUENCE, None, 0, 0, 0
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:
            for i in range(ml):
                out.append(out[start + i])
        matched += ml
    if len(out) != want:
        return E_SIZE, None, 0, 0, 0
    return OK, bytes(out), seqs, lits, matched


def decode(frame, out_bytes: int):
    """-> (the bytes or None, the result)"""
    z = bytes(frame)
    res = dict.fromkeys(DECODE_FIELDS, 0)
    res["bytes_in"] = len(z)

    def fail(status, block):
        bad = dict.fromkeys(DECODE_FIELDS, 0)
        bad.update(bytes_in=len(z), status=status, bad_block=block, content_checksum=res["content_checksum"])
        return None, bad
    status, pos, bsum, csum = parse_header(z, out_bytes)
    if status:
        return fail(status, 0)
    res["content_checksum"] = csum
    blocks = (out_bytes + BLOCK - 1)//BLOCK
    out = []
    for b in range(blocks):
        want = min(BLOCK, out_bytes - b*BLOCK)
        if pos + 4 > len(z):
            return fail(E_BLOCKS, b)
        word = struct.unpack_from("<I", z, pos)[0]
        if word == 0:
            return fail(E_SIZE, b)
        size, raw = word & 0x7FFFFFFF, word >> 31
        if size > BLOCK or size == 0 or pos + 4 + size + 4*bsum > len(z):
            return fail(E_BLOCKS, b)
        body = z[pos + 4:pos + 4 + size]
        pos += 4 + size
        if bsum:
            if struct.unpack_from("<I", z, pos)[0] != xxh32(body):
                return fail(E_CHECKSUM, b)
            pos += 4
        if raw:
            if size != want:
                return fail(E_SIZE, b)
            out.append(body)
            res["blocks_stored"] += 1
        else:
            status, data, seqs, lits, matched = decode_block(body, want)
            if status:
                return fail(status, b)
            out.append(data)
            res["blocks_compressed"] += 1
            res["sequences"] += seqs
            res["literals"] += lits
            res["matched_bytes"] += matched
    if pos + 4 > len(z) or z[pos:pos + 4] != b"\x00\x00\x00\x00":
        return fail(E_BLOCKS, blocks)
    pos += 4 + 4*csum
    if pos != len(z):
        return fail(E_BLOCKS, blocks)
    res["bytes_out"] = out_bytes
    return b"".join(out), res
