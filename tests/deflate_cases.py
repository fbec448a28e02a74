"""The inputs the zlib encoder is tested on (tests/test_deflate_ref.py on the CPU, tests/test_gpu_deflate.py on the GPU),
the twin's result for each computed once per process, and the histograms the code builder is tested on alone.

Contents (each cut to every size of SIZES it reaches):
  random     uniform bytes: stored wins
  zeros      distance 1, chains of length 258
  text       six symbols with skewed frequencies
  odd        one distinct byte and one odd byte
  no4gram    bytes in which no 4-gram repeats inside the window: no distance code is used
  fib        a Fibonacci-frequency byte multiset (22 terms, 46367 bytes), shuffled
  fib spread the same kind of multiset (18 terms, 19 with the end-of-block symbol) shuffled and spread out: one byte of it in front of every three bytes
             of a counter that makes every 4-gram unique
  BC1, BC7   oracle payloads at Quality.Normal of a 256 x 256 synth.photo
  BC1 rdo    the BC1 payload after rdo_ref at lambda 4

Why `fib spread` exists.  Shuffled, a Fibonacci multiset's frequent bytes repeat their 4-grams everywhere, the parse
turns them into matches, and the literal counts that are left are nearly flat at the top: the unlimited Huffman depth
of `fib`'s literal/length histogram is 13 (21 for the raw byte counts), and 14 at most for 23 to 25 terms, so on it the
15-bit limiter never runs.  Spread out, nothing matches, every byte stays a literal, and the depth is above 15:
test_deflate_ref.py asserts it, so the limiter cannot go untested silently."""
import functools

import numpy as np

import deflate_ref as D
import lzsize_ref as Z

SIZES = (0, 1, 3, 4, 5, 4095, 4096, 4097, 65535, 65536, 65537, 200*1024)
BIG = SIZES[-1]


def fibonacci(terms):
    f = [1, 1]
    while len(f) < terms:
        f.append(f[-1] + f[-2])
    return f[:terms]


def _fib_multiset(terms, seed, first=0):
    a = np.concatenate([np.full(c, i, np.uint8) for i, c in enumerate(fibonacci(terms)[first:])])
    np.random.default_rng(seed).shuffle(a)
    return a


def _no4gram(n, seed):
    """every 3 bytes: a random byte below 128 and a 14-bit counter in two bytes of 128 and above.  A 4-gram shows where
    in its triple it starts and holds a whole counter, and the counter's period, 49152 bytes, is longer than the window"""
    g = np.arange((n + 2)//3)
    i = g % 16384
    a = np.stack([np.random.default_rng(seed).integers(0, 128, g.size), 128 | (i >> 7), 128 | (i & 127)], axis=1)
    return a.astype(np.uint8).reshape(-1)[:n]


def _fib_spread():
    """The terms 1, 2, 3, 5, ... 4181 (the end-of-block symbol is the sequence's other 1: one 1 more and two chains
    would share the depth), 10944 bytes, each in front of its index in three digits of base 23 (bytes 32 ... 54): 43776
    bytes, one block.  A 4-gram shows where in its group it starts and holds the index's three digits (the lowest of one group
    with the higher two of the next determine it as well), so none repeats.  The 23 digit bytes occur about 1428 times
    each: the sixteen Fibonacci counts below that chain undisturbed."""
    f = _fib_multiset(19, 3, first=1)
    i = np.arange(f.size)
    return np.stack([f, 32 + i//529, 32 + i//23 % 23, 32 + i % 23], axis=1).astype(np.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def synthetic():
    rng = np.random.default_rng(7)
    odd = np.full(BIG, 0x41, np.uint8)
    odd[BIG//3] = 0x42
    return {
        "random": rng.integers(0, 256, BIG).astype(np.uint8),
        "zeros": np.zeros(BIG, np.uint8),
        "text": rng.choice(np.frombuffer(b"etaoin", np.uint8), BIG, p=[.5, .25, .12, .07, .04, .02]),
        "odd": odd,
        "no4gram": _no4gram(BIG, 9),
        "fib": _fib_multiset(22, 1),
        "fib spread": _fib_spread(),
    }


@functools.lru_cache(maxsize=None)
def payloads():
    import oracle_lib
    import rdo_ref
    from cuttlefish_amd import Format, Type, synth
    img = synth.photo(256, 256, seed=1)
    bc1 = oracle_lib.encode(img, int(Format.BC1_RGB), int(Type.UNorm), 2)
    bc7 = oracle_lib.encode(img, int(Format.BC7), int(Type.UNorm), 2)
    rdo, _ = rdo_ref.rdo(bc1, img, int(Format.BC1_RGB), int(Type.UNorm), 4.0)
    return {"BC1": bc1.reshape(-1).view(np.uint8), "BC7": bc7.reshape(-1).view(np.uint8),
            "BC1 rdo": np.ascontiguousarray(rdo).reshape(-1).view(np.uint8)}


CONTENTS = ("random", "zeros", "text", "odd", "no4gram", "fib", "fib spread", "BC1", "BC7", "BC1 rdo")
# the sizes a content reaches: every size of SIZES up to its own, and its own
_OWN = {"fib": 46367, "fib spread": 43776, "BC1": 32768, "BC7": 65536, "BC1 rdo": 32768}
CASES = [(c, n) for c in CONTENTS
         for n in sorted(set(s for s in SIZES if s <= _OWN.get(c, BIG)) | {_OWN.get(c, BIG)})]
IDS = ["%s-%d" % (c.replace(" ", "_"), n) for c, n in CASES]


def content(name):
    return synthetic()[name] if name in synthetic() else payloads()[name]


def data(name, n):
    a = content(name)
    assert n <= a.size, (name, n, a.size)
    return a[:n]


@functools.lru_cache(maxsize=None)
def twin(name, n):
    """-> (the stream, the result) of deflate_ref on a case, computed once per process"""
    return D.deflate(data(name, n))


# ---- histograms for the code builder alone: (name, counts, limit) ----
def _cl19():
    """19 Fibonacci-like counts, the shape of a code-length histogram whose unlimited depth is above 7"""
    return [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 1, 2, 3, 5, 8, 13, 21, 34]


HISTOGRAMS = (
    [("fibonacci %d" % t, fibonacci(t) + [0]*(286 - t), 15) for t in (2, 3, 15, 16, 17, 22)] +
    [("fibonacci 22 spread", [0, 0, 7] + [v for c in fibonacci(22) for v in (c, 0, 0)], 15),
     ("code lengths 19", _cl19(), 7),
     ("all equal 286", [5]*286, 15), ("all equal 286 at 9", [1]*286, 9),
     ("one symbol", [0]*40 + [9] + [0]*245, 15), ("one symbol, the first", [3] + [0]*29, 15),
     ("two symbols", [0, 4, 0, 0, 4] + [0]*25, 15), ("all zero", [0]*30, 15), ("all zero 19", [0]*19, 7)])
