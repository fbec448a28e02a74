"""The zlib encoder's definition (tests/deflate_ref.py) without a GPU, pinned from outside by Python's zlib: every
stream inflates to its input, carries its Adler-32 and fits the bound; the tokens are the estimate's; each form is
chosen; the limiter really runs; and the streams' size against zlib at level 9 on real payloads."""
import zlib

import numpy as np
import pytest

import deflate_cases as C
import deflate_ref as D
import lzsize_ref as Z

# (stream - estimate) / zlib-9 over the 32 rows of tools/deflate_quality.py is 0.0050 ... 0.0238
# (profiles/deflate_ratio.md): the estimator's band 0.95 ... 1.08 plus that range, its lower end rounded down and its
# upper end rounded up to the next 0.005.
BAND = (0.95 + 0.000, 1.08 + 0.025)


@pytest.mark.parametrize("name,n", C.CASES, ids=C.IDS)
def test_zlib_reads_the_twin(name, n):
    a = C.data(name, n)
    stream, res = C.twin(name, n)
    assert zlib.decompress(stream) == a.tobytes()
    assert stream[:2] == D.HEADER and int.from_bytes(stream[:2], "big") % 31 == 0
    assert res["adler32"] == zlib.adler32(a.tobytes()) == int.from_bytes(stream[-4:], "big")
    assert res["bytes_in"] == n and res["bytes_out"] == len(stream) <= D.deflate_bound(n)
    assert res["blocks_stored"] + res["blocks_fixed"] + res["blocks_dynamic"] == (n + Z.COSTBLK - 1)//Z.COSTBLK
    est = Z.lz_size(a)
    assert [res[k] for k in ("literals", "matches", "matched_bytes")] == [est[k] for k in ("literals", "matches", "matched_bytes")]
    if n >= 4096 and name not in ("random",):
        assert len(stream) >= est["est_bytes"]              # integer code lengths and headers only add


def test_every_form_and_edge_case_occurs():
    forms = {f: [c for c in C.CASES if C.twin(*c)[1]["blocks_" + f]] for f in D.FORMS}
    assert all(forms.values()), forms
    assert ("zeros", 5) in forms["fixed"] and ("random", C.BIG) in forms["stored"]
    # no match at all, yet coded with the group's own tables: no distance code is used
    res = C.twin("no4gram", C.BIG)[1]
    assert res["matches"] == 0 and res["blocks_dynamic"] == 4
    # one distinct literal, and a final short group
    res = C.twin("zeros", 65537)[1]
    assert (res["literals"], res["blocks_dynamic"], res["blocks_stored"]) == (2, 1, 1)
    assert C.twin("odd", C.BIG)[1]["blocks_dynamic"] == 4


def _ll_histogram(a):
    lits, (mp, ml, _) = Z.parse(a)
    ll = np.bincount(a[lits], minlength=286) + np.bincount(257 + Z.length_code(ml), minlength=286)
    ll[256] += 1
    return ll


def test_the_limiter_really_runs():
    a = C.data("fib spread", 43776)
    assert a.size <= Z.COSTBLK and C.twin("fib spread", 43776)[1]["blocks_dynamic"] == 1
    ll = _ll_histogram(a)
    deep = max(D.tree_depths(ll)[1])
    lengths = D.code_lengths(ll, D.LIMIT)
    assert deep > D.LIMIT and lengths.max() == D.LIMIT, deep
    # the shuffled multiset alone does not get there (deflate_cases says why): its case tests the path without repair
    assert max(D.tree_depths(_ll_histogram(C.data("fib", 46367)))[1]) <= D.LIMIT
    # a code-length histogram above 7 bits
    name, cl, limit = next(h for h in C.HISTOGRAMS if h[0] == "code lengths 19")
    assert len(cl) == 19 and limit == D.CL_LIMIT and max(D.tree_depths(cl)[1]) > D.CL_LIMIT
    assert D.code_lengths(cl, limit).max() == D.CL_LIMIT


@pytest.mark.parametrize("name,counts,limit", C.HISTOGRAMS, ids=[h[0].replace(" ", "_") for h in C.HISTOGRAMS])
def test_code_lengths(name, counts, limit):
    lengths = D.code_lengths(counts, limit).astype(np.int64)
    used = lengths[lengths > 0]
    assert used.size >= 2 and used.max() <= limit
    assert int((1 << (limit - used)).sum()) == 1 << limit            # a complete code: zlib accepts nothing less
    assert all(lengths[i] for i, c in enumerate(counts) if c)
    assert sum(1 for c in counts if c) >= 2 or used.size == 2
    # no symbol has a longer code than a rarer one
    order, _ = D.tree_depths(counts)
    assert all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]))
    codes = D.canonical_codes(lengths)
    seen = set()
    for c, l in zip(codes, lengths):
        if l:
            bits = format(c, "0%db" % l)[::-1]
            assert not any(bits.startswith(s) or s.startswith(bits) for s in seen)
            seen.add(bits)
    if max(D.tree_depths(counts)[1]) <= limit:
        # within the limit the lengths cost what Huffman's tree costs
        padded = D._padded(counts)
        cost = sum(padded[s]*d for s, d in zip(*D.tree_depths(counts)))
        assert sum(int(c)*int(l) for c, l in zip(padded, lengths)) == cost


def test_size_against_zlib_9():
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import deflate_quality
    rows = deflate_quality.rows()
    assert len(rows) == 32
    for name, n, z9, z1, est, size, res in rows:
        print("%-24s zlib-9 %7d  zlib-1 %7d  estimate %7d  stream %7d  ratio %.4f  addend %.4f" % (
            name, z9, z1, est, size, size/z9, (size - est)/z9))
    for name, n, z9, z1, est, size, res in rows:
        assert z9 >= 4096
        assert BAND[0] <= size/z9 <= BAND[1], (name, z9, size, size/z9)
