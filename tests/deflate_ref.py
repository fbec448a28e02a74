"""The zlib stream of a byte stream in numpy -- THE DEFINITION of the bytes csrc/deflate.hip writes (DESIGN.md section
4.16).  Every constant has its twin in csrc/deflate.h.  The stream, its matches, its parse and deflate's code tables are
lzsize_ref's: the tokens written are exactly the tokens the estimate prices.

  * wrapper: 78 9C (FCHECK valid), the block groups, the big-endian Adler-32 of the stream.  A stream of 0 bytes is
    EMPTY: the header, one final empty stored block, Adler-32 = 1.
  * one block group per COSTBLK = 65536 input bytes, every group starting on a byte boundary.  Its form is the one of
    fewest BYTES, ties in the order stored, fixed, dynamic:
      stored   one stored block per STORED_SPLIT = 32768 bytes (1 header byte, LEN, NLEN, the bytes); the last one of
               the stream carries BFINAL;
      fixed    3 header bits (BFINAL 0, BTYPE 01), the tokens with RFC 1951's fixed codes, the end-of-block code, then
               the CLOSING block: an empty stored block (3 header bits, zero bits up to the byte, 00 00 FF FF), which
               carries BFINAL in the last group;
      dynamic  the same with BTYPE 10, the code-table header and the group's own codes.
  * code lengths of an alphabet from its counts, code_lengths(counts, limit): while fewer than two symbols are used the
    lowest unused symbol counts once; the used symbols are ordered by (count, symbol); Huffman's merge by two queues
    (leaves in that order, internal nodes in the order they are made), taking the lighter front, the leaf on a tie;
    leaf depths above the limit are set to the limit; n[l] = leaves of length l; while the Kraft sum exceeds 1 (each
    step lowers it by 2^-limit): with l the largest length below the limit that has a leaf, n[l] -= 1, n[l + 1] += 2,
    n[limit] -= 1; finally the lengths are dealt in the order of the symbols, longest first: n[limit] symbols get the
    limit, the next n[limit - 1] one less, and so on.  Limits: 15 for both alphabets, 7 for the code-length alphabet.
  * codes are canonical (RFC 1951, 3.2.2).
  * the header (3.2.7): HLIT and HDIST trimmed to the last used symbol (at least 257 and 1); the lengths of both
    alphabets are ONE sequence, so a run may cross from the literal/length lengths into the distance lengths; at
    index i with value v and r equal values from i on: v = 0 and r >= 3 writes 18 (r >= 11) or 17 for min(r, 138)
    entries; v > 0, r >= 3 and the entry before i equal to v writes 16 for min(r, 6) entries; anything else writes v
    itself.  HCLEN is trimmed to the last used code-length symbol in RFC order, at least 4.

deflate_bound(n) bounds the stream's bytes; literals, matches and matched_bytes are lzsize_ref.lz_size's."""
import zlib

import numpy as np

import lzsize_ref as Z

STORED_SPLIT = 32768   # bytes per stored block                      (CFDF_STORED_SPLIT)
LIMIT = 15             # longest literal/length and distance code    (CFDF_LIMIT)
CL_LIMIT = 7           # longest code-length code                    (CFDF_CL_LIMIT)
HEADER = b"\x78\x9c"
EMPTY = HEADER + b"\x01\x00\x00\xff\xff" + b"\x00\x00\x00\x01"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FORMS = ("stored", "fixed", "dynamic")

FIELDS = ("bytes_in", "bytes_out", "blocks_stored", "blocks_fixed", "blocks_dynamic", "literals", "matches",
          "matched_bytes", "adler32", "reserved")

FIXED_LL = np.array([8]*144 + [9]*112 + [7]*24 + [8]*8, np.int64)
FIXED_DD = np.full(32, 5, np.int64)


def deflate_bound(n: int) -> int:
    """bytes that hold the stream of any n input bytes: stored groups throughout, and the empty stream's 11"""
    return 11 + n + 10*((n + Z.COSTBLK - 1)//Z.COSTBLK)


def _padded(counts):
    c = [int(v) for v in counts]
    while sum(1 for v in c if v) < 2:
        c[next(i for i, v in enumerate(c) if not v)] = 1
    return c


def tree_depths(counts):
    """-> (symbols in (count, symbol) order, their depths in the unlimited Huffman tree)"""
    c = _padded(counts)
    order = sorted((i for i, v in enumerate(c) if v), key=lambda i: (c[i], i))
    m = len(order)
    weight = [c[i] for i in order] + [0]*(m - 1)         # node j < m: leaf; m + k: the k-th internal node
    parent = [0]*(2*m - 1)
    leaf, node = 0, m
    for k in range(m - 1):
        pick = []
        for _ in range(2):
            if leaf < m and (node >= m + k or weight[leaf] <= weight[node]):
                pick.append(leaf)
                leaf += 1
            else:
                pick.append(node)
                node += 1
        weight[m + k] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = m + k
    depth = [0]*(2*m - 1)
    for j in range(2*m - 3, -1, -1):
        depth[j] = depth[parent[j]] + 1
    return order, depth[:m]


def code_lengths(counts, limit):
    """-> the code length of every symbol (uint8 array), lengths <= limit, Kraft sum exactly 1"""
    order, depth = tree_depths(counts)
    n = [0]*(limit + 1)
    for d in depth:
        n[min(d, limit)] += 1
    kraft = sum(n[l] << (limit - l) for l in range(1, limit + 1))
    while kraft > 1 << limit:
        l = limit - 1
        while not n[l]:
            l -= 1
        n[l] -= 1
        n[l + 1] += 2
        n[limit] -= 1
        kraft -= 1
    lengths = np.zeros(len(counts), np.uint8)
    at = 0
    for l in range(limit, 0, -1):
        for s in order[at:at + n[l]]:
            lengths[s] = l
        at += n[l]
    return lengths


def canonical_codes(lengths):
    """-> the codes of RFC 1951 3.2.2, bit-reversed: the way they enter the stream, first bit lowest"""
    lengths = [int(v) for v in lengths]
    top = max(lengths + [1])
    n = [0]*(top + 2)
    for l in lengths:
        if l:
            n[l] += 1
    code, nxt = 0, [0]*(top + 2)
    for l in range(1, top + 1):
        code = (code + n[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append(0)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(int(format(c, "0%db" % l)[::-1], 2))
    return out


def header_tokens(ll_len, dd_len):
    """-> (hlit, hdist, [(code-length symbol, extra value, extra bits)])"""
    hlit = max(257, max(i for i, v in enumerate(ll_len) if v) + 1)
    hdist = max(1, max(i for i, v in enumerate(dd_len) if v) + 1)
    seq = [int(v) for v in ll_len[:hlit]] + [int(v) for v in dd_len[:hdist]]
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            c = min(r, 138)
            out.append((18, c - 11, 7) if c >= 11 else (17, c - 3, 3))
            i += c
        elif v and r >= 3 and i and seq[i - 1] == v:
            c = min(r, 6)
            out.append((16, c - 3, 2))
            i += c
        else:
            out.append((v, 0, 0))
            i += 1
    return hlit, hdist, out


class _Bits:
    def __init__(self):
        self.val, self.len = [], []

    def put(self, value, nbits):
        self.val.append(np.atleast_1d(np.asarray(value, np.int64)))
        self.len.append(np.atleast_1d(np.asarray(nbits, np.int64)))

    def size(self):
        return int(sum(int(v.sum()) for v in self.len))

    def bytes(self):
        val, ln = np.concatenate(self.val), np.concatenate(self.len)
        at = np.cumsum(ln) - ln
        bits = np.zeros((int(ln.sum()) + 7)//8*8, np.uint8)
        for b in range(int(ln.max())):
            m = ln > b
            bits[at[m] + b] = (val[m] >> b) & 1
        return np.packbits(bits, bitorder="little").tobytes()


def _closing(bits: _Bits, final: bool):
    bits.put(1 if final else 0, 3)
    bits.put(0, -bits.size() % 8)
    bits.put(0xFFFF0000, 32)


def _group(a, lo, hi, lits, mats, final):
    """the bytes of one group and its form; lits: positions, mats: (positions, lengths, distances), all inside it"""
    mp, ml, md = mats
    lc, dc = Z.length_code(ml), Z.dist_code(md)
    le, de = np.asarray(Z.LEN_EXTRA)[lc], np.asarray(Z.DIST_EXTRA)[dc]
    ll = np.bincount(a[lits], minlength=286).astype(np.int64) + np.bincount(257 + lc, minlength=286)
    ll[256] += 1
    dd = np.bincount(dc, minlength=30).astype(np.int64)
    extra = int(le.sum() + de.sum())
    n = hi - lo
    stored = n + 5*(1 + (n > STORED_SPLIT))
    fixed_bits = 3 + int((ll*FIXED_LL[:286]).sum()) + 5*int(dd.sum()) + extra
    ll_len, dd_len = code_lengths(ll, LIMIT), code_lengths(dd, LIMIT)
    hlit, hdist, toks = header_tokens(ll_len, dd_len)
    cl = np.bincount([t[0] for t in toks], minlength=19)
    cl_len = code_lengths(cl, CL_LIMIT)
    hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_len[s]) + 1)
    head_bits = 3 + 14 + 3*hclen + sum(int(cl_len[s]) + eb for s, _, eb in toks)
    dyn_bits = head_bits + int((ll*ll_len.astype(np.int64)).sum() + (dd*dd_len.astype(np.int64)).sum()) + extra
    sizes = (stored, (fixed_bits + 3 + 7)//8 + 4, (dyn_bits + 3 + 7)//8 + 4)
    form = sizes.index(min(sizes))
    if form == 0:
        out = b""
        for s in range(lo, hi, STORED_SPLIT):
            e = min(hi, s + STORED_SPLIT)
            out += bytes([1 if final and e == hi else 0]) + (e - s).to_bytes(2, "little") + \
                ((e - s) ^ 0xFFFF).to_bytes(2, "little") + a[s:e].tobytes()
        assert len(out) == stored
        return out, form
    bits = _Bits()
    if form == 1:
        bits.put(2, 3)                                    # BFINAL 0, BTYPE 01
        llc, ddc = canonical_codes(FIXED_LL), canonical_codes(FIXED_DD)
        ll_len, dd_len = FIXED_LL, FIXED_DD
    else:
        bits.put(4, 3)                                    # BFINAL 0, BTYPE 10
        bits.put(hlit - 257, 5)
        bits.put(hdist - 1, 5)
        bits.put(hclen - 4, 4)
        bits.put([int(cl_len[s]) for s in CL_ORDER[:hclen]], [3]*hclen)
        clc = canonical_codes(cl_len)
        for s, ev, eb in toks:
            bits.put(clc[s] | (ev << int(cl_len[s])), int(cl_len[s]) + eb)
        assert bits.size() == head_bits
        llc, ddc = canonical_codes(ll_len), canonical_codes(dd_len)
    llc, ddc = np.asarray(llc, np.int64), np.asarray(ddc, np.int64)
    ll_len, dd_len = np.asarray(ll_len, np.int64), np.asarray(dd_len, np.int64)
    # tokens in stream order: a literal is one piece, a match two (length with its extra bits, distance with its)
    pos = np.concatenate([lits, mp, mp])
    rank = np.concatenate([np.zeros(lits.size, np.int64), np.zeros(mp.size, np.int64), np.ones(mp.size, np.int64)])
    ls = 257 + lc
    val = np.concatenate([llc[a[lits]], llc[ls] | ((ml - np.asarray(Z.LEN_BASE)[lc]) << ll_len[ls]),
                          ddc[dc] | ((md - np.asarray(Z.DIST_BASE)[dc]) << dd_len[dc])])
    ln = np.concatenate([ll_len[a[lits]], ll_len[ls] + le, dd_len[dc] + de])
    o = np.lexsort((rank, pos))
    bits.put(val[o], ln[o])
    bits.put(llc[256], ll_len[256])
    assert bits.size() == (fixed_bits, dyn_bits)[form - 1]
    _closing(bits, final)
    out = bits.bytes()
    assert len(out) == sizes[form]
    return out, form


def deflate(spans):
    """-> (the zlib stream, the fields of cfhip_deflate_result)"""
    a = Z.stream(spans)
    n = a.size
    assert n < 1 << 31
    res = dict.fromkeys(FIELDS, 0)
    res["bytes_in"] = n
    res["adler32"] = zlib_adler(a)
    if not n:
        res["bytes_out"] = len(EMPTY)
        return EMPTY, res
    lits, (mp, ml, md) = Z.parse(a)
    out = [HEADER]
    groups = (n + Z.COSTBLK - 1)//Z.COSTBLK
    for g in range(groups):
        lo, hi = g*Z.COSTBLK, min(n, (g + 1)*Z.COSTBLK)
        mi = (mp >= lo) & (mp < hi)
        part, form = _group(a, lo, hi, lits[(lits >= lo) & (lits < hi)], (mp[mi], ml[mi], md[mi]), g == groups - 1)
        out.append(part)
        res["blocks_" + FORMS[form]] += 1
    out.append(res["adler32"].to_bytes(4, "big"))
    out = b"".join(out)
    res.update(bytes_out=len(out), literals=int(lits.size), matches=int(mp.size), matched_bytes=int(ml.sum()))
    assert len(out) <= deflate_bound(n)
    return out, res


def zlib_adler(a) -> int:
    """Adler-32 by its definition (RFC 1950), in chunks the way the kernels combine it"""
    A, B = 1, 0
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8).astype(np.int64)
    for s in range(0, b.size, Z.CHUNK):
        c = b[s:s + Z.CHUNK]
        B = (B + c.size*A + int((c*np.arange(c.size, 0, -1)).sum())) % 65521
        A = (A + int(c.sum())) % 65521
    return (B << 16) | A


def twin(spans) -> bytes:
    return deflate(spans)[0]


if __name__ == "__main__":
    x = np.random.default_rng(0).integers(0, 6, 100000).astype(np.uint8)
    s, r = deflate(x)
    assert zlib.decompress(s) == x.tobytes()
    print(r)
