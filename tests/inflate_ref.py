"""Indexed inflate of zlib streams in plain Python -- THE DEFINITION of what csrc/inflate.hip and csrc/inflate.h compute
(DESIGN.md section 4.17): the index of a stream, the verdict (status, bad_chunk) on a stream with an index, and the
counters of cfhip_inflate_result.  Written from RFC 1950 / RFC 1951; zlib is not used.

Bits are numbered from the start of the zlib stream: bit k is bit k & 7 of byte k >> 3.  The index of a stream whose
output is n bytes has C = ceil(n / 4096) entries (header_bit, token_bit): header_bit is the BFINAL bit of the deflate
block that holds output byte 4096 c, token_bit the first bit of the literal/length code of the token that produces that
byte (in a stored block: 8 x the position of that data byte).  A stream is INDEXABLE when every output position 4096 c
is the first byte of a token; build_index raises NotIndexable otherwise.

The rules of the format:
  * wrapper: at least 6 bytes; the low four bits of CMF are 8; (CMF x 256 + FLG) % 31 == 0; no FDICT; the stream is
    EXACTLY its length: behind the block with BFINAL come the padding bits up to the byte, the big-endian Adler-32,
    and nothing.
  * a block header: BTYPE 3 is an error; a stored block's LEN must be the complement of NLEN; a dynamic header is
    rejected when HLIT > 286 or HDIST > 30, when a repeat code (16) comes first or a run goes past HLIT + HDIST, when
    symbol 256 has length 0, or when one of the three codes has a Kraft sum above 1.  An INCOMPLETE code is accepted.
  * a bit pattern that belongs to no code is a code error; so are literal/length symbols 286 and 287 and distance
    codes 30 and 31.  A symbol is decoded from the next 15 bits, the stream continued with zeros: a code that ends
    behind the stream's last bit is an overrun, and so is "no code" when fewer than 15 bits were left.
  * a distance that reaches before output byte 0 is a distance error.

The seven error classes (cfhip_inflate_status): 1 wrapper, 2 index, 3 block header, 4 code, 5 distance, 6 overrun (the
stream, or its BFINAL block, ends before the output does), 7 checksum.

WHAT A CHUNK CHECKS, and in which order -- inflate_indexed(stream, index, n).  Chunk c (want = min(4096, n - 4096 c)
bytes) runs on its own; the verdict is that of the LOWEST failing chunk:
  1. chunk 0: the wrapper's first two bytes; then the walk from bit 16 through everything that produces no output
     (end-of-block codes, empty blocks of any type and their headers) to the first token that produces output: the
     block it lies in and its bit must be entry 0 (else index; the stream ending first is an overrun).
     chunk c > 0: 16 <= header_bit < token_bit <= 8 x bytes (else index); the header at header_bit is parsed; a
     token_bit before the header's end (stored: not a data byte of that block) is an index error.
  2. tokens are read until exactly `want` bytes are produced.  Per match, in this order: code errors, the distance
     check, then a match that would run past `want`: an index error.  A block that ends is followed by the next
     header; a BFINAL block that ends here is an overrun.
  3. the walk through everything that produces no output.  It stops in front of a token that produces output: for
     the last chunk that is an index error (the stream holds more than n bytes), otherwise the block and the bit
     must be entry c + 1 (else index).  It ends with the BFINAL block: an overrun unless c is the last chunk, which
     then checks that the trailer's four bytes end the stream (else wrapper).
  4. when every chunk passed, the Adler-32 of the output is compared with the trailer's (checksum, reported at the
     last chunk).
With n == 0 there are no chunks: steps 1 and 3 run as one walk from bit 16 (reported at chunk 0), then step 4.

By induction from bit 16 a stream that passes is a valid zlib stream of exactly n bytes: the index is validated, not
trusted."""

CHUNK = 4096                        # output bytes per index entry (CFLZ_CHUNK)
OK, E_WRAPPER, E_INDEX, E_HEADER, E_CODE, E_DISTANCE, E_OVERRUN, E_CHECKSUM = range(8)
CLASSES = ("ok", "wrapper", "index", "block header", "code", "distance", "overrun", "checksum")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIELDS = ("bytes_in", "bytes_out", "literals", "matches", "matched_bytes", "adler32", "status", "bad_chunk", "rounds")
FIXED_LL = [8]*144 + [9]*112 + [7]*24 + [8]*8
FIXED_DD = [5]*32


class Verdict(Exception):
    """an error class, raised inside this module only"""
    def __init__(self, status):
        super().__init__(CLASSES[status])
        self.status = status


class InflateError(ValueError):
    """inflate(): the stream is no valid zlib stream"""


class NotIndexable(ValueError):
    """build_index(): a token crosses an output position 4096 c"""


def zindex_entries(n: int) -> int:
    return (n + CHUNK - 1)//CHUNK


def length_base(lc):
    """(base, extra bits) of length code 257 + lc, 0 <= lc <= 28"""
    if lc < 8:
        return 3 + lc, 0
    if lc == 28:
        return 258, 0
    e = (lc - 4) >> 2
    return 3 + ((4 + (lc & 3)) << e), e


def dist_base(dc):
    """(base, extra bits) of distance code dc, 0 <= dc <= 29"""
    if dc < 4:
        return 1 + dc, 0
    e = (dc - 2) >> 1
    return 1 + ((2 + (dc & 1)) << e), e


class _Code:
    """a canonical code from its lengths; a Kraft sum above 1 is a block header error"""
    def __init__(self, lengths):
        self.cnt = [0]*16
        for l in lengths:
            self.cnt[l] += 1
        self.cnt[0] = 0
        if sum(self.cnt[l] << (15 - l) for l in range(1, 16)) > 1 << 15:
            raise Verdict(E_HEADER)
        self.first, self.offs = [0]*16, [0]*16
        code = at = 0
        for l in range(1, 16):
            self.first[l], self.offs[l] = code, at
            code = (code + self.cnt[l]) << 1
            at += self.cnt[l]
        self.sorted = sorted((s for s, l in enumerate(lengths) if l), key=lambda s: (lengths[s], s))
        self.memo = {}

    def lookup(self, bits15):
        """-> (symbol, length) of the code that starts the 15 bits (first bit lowest), or None"""
        hit = self.memo.get(bits15, 0)
        if hit == 0:
            hit, code = None, 0
            for l in range(1, 16):
                code = (code << 1) | ((bits15 >> (l - 1)) & 1)
                if code - self.first[l] < self.cnt[l]:
                    hit = (self.sorted[self.offs[l] + code - self.first[l]], l)
                    break
            self.memo[bits15] = hit
        return hit


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_Code(FIXED_LL), _Code(FIXED_DD))
    return _FIXED


class _Reader:
    """the bits of a stream, a block at a time"""
    def __init__(self, z):
        self.z = bytes(z)
        self.T = 8*len(self.z)
        self.pos = 0
        self.hdr = 0
        self.final = self.btype = self.left = self.data = self.len = 0
        self.ll = self.dd = None

    def peek(self, k):
        p = self.pos >> 3                                        # zeros behind the stream
        return (int.from_bytes(self.z[p:p + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)

    def get(self, k):
        if self.pos + k > self.T:
            raise Verdict(E_OVERRUN)
        v = self.peek(k)
        self.pos += k
        return v

    def symbol(self, code, consume=True):
        hit = code.lookup(self.peek(15))
        if hit is None:
            raise Verdict(E_OVERRUN if self.T - self.pos < 15 else E_CODE)
        if self.pos + hit[1] > self.T:
            raise Verdict(E_OVERRUN)
        if consume:
            self.pos += hit[1]
        return hit[0]

    def header(self):
        """the block header at pos; afterwards pos is the block's first token (stored: its first data byte)"""
        self.hdr = self.pos
        v = self.get(3)
        self.final, self.btype = v & 1, v >> 1
        if self.btype == 3:
            raise Verdict(E_HEADER)
        if self.btype == 0:
            p = (self.pos + 7) >> 3
            if p + 4 > len(self.z):
                raise Verdict(E_OVERRUN)
            ln, nl = self.z[p] | self.z[p + 1] << 8, self.z[p + 2] | self.z[p + 3] << 8
            if ln != nl ^ 0xFFFF:
                raise Verdict(E_HEADER)
            if p + 4 + ln > len(self.z):
                raise Verdict(E_OVERRUN)
            self.data, self.len, self.left, self.pos = p + 4, ln, ln, 8*(p + 4)
        elif self.btype == 1:
            self.ll, self.dd = _fixed()
        else:
            hlit, hdist, hclen = self.get(5) + 257, self.get(5) + 1, self.get(4) + 4
            if hlit > 286 or hdist > 30:
                raise Verdict(E_HEADER)
            cl = [0]*19
            for i in range(hclen):
                cl[CL_ORDER[i]] = self.get(3)
            clc = _Code(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s = self.symbol(clc)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Verdict(E_HEADER)
                    v, r = lens[-1], 3 + self.get(2)
                elif s == 17:
                    v, r = 0, 3 + self.get(3)
                else:
                    v, r = 0, 11 + self.get(7)
                if len(lens) + r > hlit + hdist:
                    raise Verdict(E_HEADER)
                lens += [v]*r
            if not lens[256]:
                raise Verdict(E_HEADER)
            self.ll = _Code(lens[:hlit])
            self.dd = _Code(lens[hlit:])

    def token(self):
        """the next token of a fixed or dynamic block -> ("lit", byte) | ("eob",) | ("match", length, distance)"""
        s = self.symbol(self.ll)
        if s < 256:
            return ("lit", s)
        if s == 256:
            return ("eob",)
        if s >= 286:
            raise Verdict(E_CODE)
        base, e = length_base(s - 257)
        length = base + self.get(e)
        d = self.symbol(self.dd)
        if d >= 30:
            raise Verdict(E_CODE)
        base, e = dist_base(d)
        return ("match", length, base + self.get(e))

    def skip_no_output(self):
        """from inside a block: walk through everything that produces no output.  -> True in front of a token that
        produces output, False behind the end of the BFINAL block"""
        while True:
            if self.btype == 0:
                if self.left:
                    return True
            elif self.symbol(self.ll, consume=False) != 256:
                return True
            else:
                self.symbol(self.ll)
            if self.final:
                return False
            self.header()


def adler32(data) -> int:
    a, b = 1, 0
    for s in range(0, len(data), 3800):               # 3800 x 255 x 3800 stays far below any overflow worry in C
        for v in data[s:s + 3800]:
            a += v
            b += a
        a %= 65521
        b %= 65521
    return (b << 16) | a


def _wrapper_head(z):
    if len(z) < 6 or (z[0] & 15) != 8 or (z[0]*256 + z[1]) % 31 or z[1] & 0x20:
        raise Verdict(E_WRAPPER)


def _serial(z, on_token=None):
    """the plain serial inflater; on_token(out position, header bit, token bit, bytes produced) per token"""
    z = bytes(z)
    _wrapper_head(z)
    r = _Reader(z)
    r.pos = 16
    out = bytearray()
    while True:
        r.header()
        if r.btype == 0:
            for i in range(r.len):
                if on_token:
                    on_token(len(out), r.hdr, 8*(r.data + i), 1)
                out.append(z[r.data + i])
            r.pos += 8*r.len
        else:
            while True:
                at = r.pos
                t = r.token()
                if t[0] == "eob":
                    break
                if on_token:
                    on_token(len(out), r.hdr, at, 1 if t[0] == "lit" else t[1])
                if t[0] == "lit":
                    out.append(t[1])
                else:
                    if t[2] > len(out):
                        raise Verdict(E_DISTANCE)
                    for _ in range(t[1]):
                        out.append(out[-t[2]])
        if r.final:
            break
    p = (r.pos + 7) >> 3
    if p + 4 != len(z):
        raise Verdict(E_WRAPPER)
    if int.from_bytes(z[p:], "big") != adler32(out):
        raise Verdict(E_CHECKSUM)
    return bytes(out)


def inflate(stream) -> bytes:
    """the bytes of a zlib stream; InflateError where it is none by the rules above"""
    try:
        return _serial(stream)
    except Verdict as v:
        raise InflateError(CLASSES[v.status]) from None


def build_index(stream):
    """-> [(header_bit, token_bit)] per 4096 output bytes; NotIndexable, or InflateError for an invalid stream"""
    index = []

    def on_token(at, hdr, bit, produced):
        if at % CHUNK == 0:
            index.append((hdr, bit))
        elif at//CHUNK != (at + produced - 1)//CHUNK:
            raise NotIndexable("the token at output byte %d crosses byte %d" % (at, (at//CHUNK + 1)*CHUNK))
    inflate_out = None
    try:
        inflate_out = _serial(stream, on_token)
    except Verdict as v:
        raise InflateError(CLASSES[v.status]) from None
    assert len(index) == zindex_entries(len(inflate_out))
    return index


def _chunk(z, index, n, c, out, counts):
    """chunk c by the rules of the docstring: appends its bytes to out (which holds the chunks before it) or raises"""
    C = zindex_entries(n)
    want = min(CHUNK, n - CHUNK*c) if n else 0
    r = _Reader(z)
    if c == 0:
        _wrapper_head(z)
        r.pos = 16
        r.header()
        more = r.skip_no_output()
        if want:
            if not more:
                raise Verdict(E_OVERRUN)
            if (r.hdr, r.pos) != tuple(index[0]):
                raise Verdict(E_INDEX)
    else:
        hb, tb = index[c]
        if not 16 <= hb < tb <= r.T:
            raise Verdict(E_INDEX)
        r.pos = hb
        r.header()
        if r.btype == 0:
            if tb % 8 or not r.data <= tb//8 < r.data + r.len:
                raise Verdict(E_INDEX)
            r.left = r.len - (tb//8 - r.data)
        elif tb < r.pos:
            raise Verdict(E_INDEX)
        r.pos = tb
    produced = 0
    while produced < want:
        if r.btype == 0:
            if r.left:
                k = min(r.left, want - produced)
                out += z[r.pos >> 3:(r.pos >> 3) + k]
                r.pos += 8*k
                r.left -= k
                produced += k
                counts[0] += k
                continue
        else:
            t = r.token()
            if t[0] == "lit":
                out.append(t[1])
                produced += 1
                counts[0] += 1
                continue
            if t[0] == "match":
                if t[2] > CHUNK*c + produced:
                    raise Verdict(E_DISTANCE)
                if produced + t[1] > want:
                    raise Verdict(E_INDEX)
                for _ in range(t[1]):
                    out.append(out[-t[2]])
                produced += t[1]
                counts[1] += 1
                counts[2] += t[1]
                continue
        if r.final:
            raise Verdict(E_OVERRUN)
        r.header()
    if want:
        more = r.skip_no_output()
    if more:
        if c + 1 >= C:
            raise Verdict(E_INDEX)
        if (r.hdr, r.pos) != tuple(index[c + 1]):
            raise Verdict(E_INDEX)
        return
    if c + 1 < C:
        raise Verdict(E_OVERRUN)
    if ((r.pos + 7) >> 3) + 4 != len(z):
        raise Verdict(E_WRAPPER)


def inflate_indexed(stream, index, n):
    """-> (the n bytes or None, the fields of cfhip_inflate_result without `rounds`)"""
    z = bytes(stream)
    index = [(int(a), int(b)) for a, b in index]
    C = zindex_entries(n)
    assert len(index) >= C
    res = dict.fromkeys(FIELDS[:-1], 0)
    res["bytes_in"] = len(z)
    out, counts = bytearray(), [0, 0, 0]
    for c in range(max(C, 1)):
        try:
            _chunk(z, index, n, c, out, counts)
        except Verdict as v:
            res.update(status=v.status, bad_chunk=c)
            return None, res
    a = adler32(out)
    if int.from_bytes(z[-4:], "big") != a:
        res.update(status=E_CHECKSUM, bad_chunk=max(C, 1) - 1)
        return None, res
    res.update(bytes_out=n, literals=counts[0], matches=counts[1], matched_bytes=counts[2], adler32=a)
    return bytes(out), res
