"""The deflate-size estimate of a byte stream in numpy -- THE DEFINITION of what csrc/lzsize.hip computes
(DESIGN.md section 4.15).  Every constant has its twin in csrc/lzsize.h.

The stream a[0..N), N < 2^31 (several spans: their concatenation), is parsed into literals and matches and priced with
the zeroth-order entropy of deflate's two alphabets:

  * key(p): the little-endian 32-bit word at p <= N - 4.  The candidates of p are the up to K largest q < p with
    key(q) == key(p) and p - q <= W, nearest first;
  * end(p) = min(N, (p // CHUNK + 1) CHUNK); len_j = min(common prefix of a[p:] and a[q_j:], MAX, end(p) - p), the
    prefix running past p where it does (overlapping matches); L(p) = max_j len_j, D(p) = p - q_j for the smallest j
    reaching it; L(p) = 0 without a candidate or for p > N - 4;
  * parse, per chunk, p from its start: l = L(p); if l >= MIN and p + 1 < end(p) and L(p + 1) > l then l = 0 (one-step
    lazy); l >= MIN emits the match (l, D(p)) and p += l, otherwise the literal a[p] and p += 1;
  * cost, per block of COSTBLK input bytes: histogram ll[286] (literals, one end-of-block symbol 256, 257 + deflate's
    length code), dd[30] (deflate's distance code), extra = the extra bits of both (RFC 1951, tables below);
    bits_q16 = sum n (lg16(T_ll) - lg16(n)) over ll + the same over dd + (extra << 16); no header term;
  * lg16: log2 in 16.16 fixed point, integers only (below).

Every quantity is an integer sum: the kernels return these numbers exactly."""
import numpy as np

MIN = 4             # shortest match                         (CFLZ_MIN)
MAX = 258           # longest match                          (CFLZ_MAX)
W = 32768           # window                                 (CFLZ_WINDOW)
K = 4               # candidates per position                (CFLZ_CANDS)
CHUNK = 4096        # bytes parsed independently             (CFLZ_CHUNK)
COSTBLK = 65536     # bytes priced with one pair of tables   (CFLZ_COSTBLK)

FIELDS = ("bytes_in", "bits_q16", "est_bytes", "literals", "matches", "matched_bytes")

# RFC 1951, section 3.2.5: length codes 257..285 and distance codes 0..29
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def length_code(length):
    """deflate's length code minus 257 for lengths 3..258 (array or scalar)"""
    return np.searchsorted(np.asarray(LEN_BASE), length, side="right") - 1


def dist_code(dist):
    """deflate's distance code for distances 1..32768"""
    return np.searchsorted(np.asarray(DIST_BASE), dist, side="right") - 1


def lg16(x: int) -> int:
    """log2(x) in 16.16 fixed point for an integer x >= 1, by sixteen squarings of a 32-bit mantissa"""
    x = int(x)
    assert x >= 1
    e = x.bit_length() - 1
    m = x << (31 - e)
    f = 0
    for _ in range(16):
        m = (m*m) >> 31
        if m >= 1 << 32:
            f = 2*f + 1
            m >>= 1
        else:
            f = 2*f
    return (e << 16) | f


def stream(spans) -> np.ndarray:
    if isinstance(spans, (bytes, bytearray, np.ndarray)):
        spans = [spans]
    parts = [np.frombuffer(bytes(s), np.uint8) if isinstance(s, (bytes, bytearray))
             else np.ascontiguousarray(s).reshape(-1).view(np.uint8) for s in spans]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def matches(a: np.ndarray):
    """-> (L, D) of every position, int32"""
    n = a.size
    L = np.zeros(n, np.int32)
    D = np.zeros(n, np.int32)
    if n < 5:
        return L, D
    b = a.astype(np.uint32)
    keys = b[:n - 3] | (b[1:n - 2] << 8) | (b[2:n - 1] << 16) | (b[3:] << 24)
    order = np.argsort(keys, kind="stable").astype(np.int64)
    sk = keys[order]
    pad = np.concatenate([a, np.zeros(MAX + 1, np.uint8)])
    alive = np.ones(order.size, bool)               # the walk towards earlier entries has not stopped
    for j in range(1, K + 1):
        alive[:j] = False
        alive[j:] &= (sk[j:] == sk[:-j]) & (order[j:] - order[:-j] <= W)
        idx = np.nonzero(alive)[0]
        if not idx.size:
            break
        p, q = order[idx], order[idx - j]
        cap = np.minimum(MAX, np.minimum(n, (p//CHUNK + 1)*CHUNK) - p)
        ln = np.zeros(idx.size, np.int64)
        act = np.nonzero(ln < cap)[0]
        while act.size:
            same = pad[p[act] + ln[act]] == pad[q[act] + ln[act]]
            act = act[same]
            ln[act] += 1
            act = act[ln[act] < cap[act]]
        better = ln > L[p]                          # a later (farther) candidate wins only when strictly longer
        L[p[better]] = ln[better]
        D[p[better]] = (p - q)[better]
    return L, D


def parse(a: np.ndarray, L=None, D=None):
    """-> (positions of the literals, (position, length, distance) of the matches), int64 arrays"""
    if L is None:
        L, D = matches(a)
    n = a.size
    Ll = L.tolist()
    lits, mats = [], []
    p = 0
    while p < n:
        end = min(n, (p//CHUNK + 1)*CHUNK)
        while p < end:
            l = Ll[p]
            if l >= MIN and p + 1 < end and Ll[p + 1] > l:
                l = 0
            if l >= MIN:
                mats.append(p)
                p += l
            else:
                lits.append(p)
                p += 1
    lits = np.asarray(lits, np.int64)
    mats = np.asarray(mats, np.int64)
    return lits, (mats, L[mats].astype(np.int64), D[mats].astype(np.int64))


def entropy_q16(hist) -> int:
    total = int(sum(int(v) for v in hist))
    if not total:
        return 0
    lt = lg16(total)
    return sum(int(v)*(lt - lg16(int(v))) for v in hist if v)


def lz_size(spans) -> dict:
    """The six numbers of cfhip_lz_stats for the concatenation of the spans"""
    a = stream(spans)
    n = a.size
    assert n < 1 << 31
    out = dict.fromkeys(FIELDS, 0)
    out["bytes_in"] = n
    if not n:
        return out
    lits, (mp, ml, md) = parse(a)
    lc, dc = length_code(ml), dist_code(md)
    extra = np.asarray(LEN_EXTRA)[lc] + np.asarray(DIST_EXTRA)[dc]
    bits = 0
    for blk in range((n + COSTBLK - 1)//COSTBLK):
        lo, hi = blk*COSTBLK, (blk + 1)*COSTBLK
        li = lits[(lits >= lo) & (lits < hi)]
        mi = (mp >= lo) & (mp < hi)
        ll = np.bincount(a[li], minlength=286).astype(np.int64)
        ll += np.bincount(257 + lc[mi], minlength=286)
        ll[256] += 1
        dd = np.bincount(dc[mi], minlength=30)
        bits += entropy_q16(ll) + entropy_q16(dd) + (int(extra[mi].sum()) << 16)
    out["bits_q16"] = bits
    out["est_bytes"] = (bits + (8 << 16) - 1)//(8 << 16)
    out["literals"] = int(lits.size)
    out["matches"] = int(mp.size)
    out["matched_bytes"] = int(ml.sum())
    return out
