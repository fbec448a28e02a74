"""The definition of the indexed inflate, tests/inflate_ref.py, on the CPU: the encoder's own streams round-trip through
it, an independent encoder's flushed streams are indexable and round-trip, an unflushed one is not indexable, and on
the mutation corpus (tests/inflate_cases.py) it never raises anything but its own verdict, accepts only what zlib
accepts, and meets every one of its seven error classes.

The counters of a passing stream are deflate_ref's, with the bytes of STORED groups read as literals (a stored group
holds no tokens; inflate_cases.counts_read says why random-204800 differs from deflate_ref's own counts)."""
import zlib

import pytest

import deflate_cases as C
import inflate_cases as IC
import inflate_ref as I


@pytest.mark.parametrize("name,n", C.CASES, ids=C.IDS)
def test_own_streams_round_trip(name, n):
    x = C.data(name, n).tobytes()
    stream, res = C.twin(name, n)
    assert I.inflate(stream) == x
    index = IC.own_index(name, n)
    assert len(index) == I.zindex_entries(n) == (n + 4095)//4096
    out, got = IC.own_verdict(name, n)
    assert out == x and got["status"] == 0 and got["bad_chunk"] == 0
    assert (got["bytes_in"], got["bytes_out"]) == (len(stream), n)
    want = IC.counts_read(name, n)
    assert {k: got[k] for k in want} == want
    if not res["blocks_stored"]:
        assert {k: got[k] for k in want} == {k: res[k] for k in want}       # deflate_ref's own, unchanged


@pytest.mark.parametrize("content,n,mode", IC.FOREIGN, ids=IC.FOREIGN_IDS)
def test_foreign_streams_are_indexable(content, n, mode):
    x, z, index = IC.foreign(content, n, mode)
    assert zlib.decompress(z) == x and len(x) == n
    assert I.inflate(z) == x
    assert len(index) == I.zindex_entries(n)
    out, got = IC.foreign_verdict(content, n, mode)
    assert out == x and got["status"] == 0 and got["adler32"] == zlib.adler32(x)
    assert got["literals"] + got["matched_bytes"] == n


def test_unflushed_stream_is_not_indexable():
    z = zlib.compress(C.data("text", 20000).tobytes(), 9)
    assert I.inflate(z) == C.data("text", 20000).tobytes()
    with pytest.raises(I.NotIndexable):
        I.build_index(z)


def test_empty_streams():
    import deflate_ref
    for z in (deflate_ref.EMPTY, zlib.compress(b"")):
        assert I.inflate(z) == b"" and I.build_index(z) == []
        out, got = I.inflate_indexed(z, [], 0)
        assert out == b"" and got["status"] == 0 and got["adler32"] == 1
    assert I.inflate_indexed(deflate_ref.EMPTY + b"\x00", [], 0)[1]["status"] == I.E_WRAPPER
    assert I.inflate_indexed(C.twin("text", 5)[0], [], 0)[1]["status"] == I.E_INDEX


def test_mutations():
    for tag, z, index, n, x in IC.originals():
        out, got = I.inflate_indexed(z, index, n)
        assert out == x and got["status"] == 0, tag
    seen, accepted = set(), 0
    for (label, z, index, n), (out, got) in zip(IC.mutations(), IC.verdicts()):
        seen.add(got["status"])
        assert 0 <= got["status"] <= 7 and 0 <= got["bad_chunk"] < max(I.zindex_entries(n), 1), label
        if out is None:
            assert got["status"] != 0 and got["bytes_out"] == 0, label
            continue
        # whatever the twin accepts, zlib accepts, with the same bytes
        accepted += 1
        assert got["status"] == 0 and zlib.decompress(z) == out and len(out) == n, label
    assert seen >= set(range(1, 8)), sorted(seen)           # no class goes untested
    assert accepted >= 1
    # the record the GPU test reads instead of running the twin again
    assert IC.recorded_verdicts() == [(label, got["status"], got["bad_chunk"])
                                      for (label, _, _, _), (_, got) in zip(IC.mutations(), IC.verdicts())]
