"""The decode logic the kernels run (csrc/inflate.h) on the CPU: tools/inflate_host.cpp, built with the host compiler
alone, on the whole corpus -- the encoder's own streams, the foreign streams and every mutation -- against the
definition, tests/inflate_ref.py: (status, bad_chunk, adler32) and the counters, record by record."""
import os
import shutil
import subprocess

import pytest

import deflate_cases as C
import inflate_cases as IC
import inflate_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_program_matches_the_twin(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path/"inflate_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "inflate_host.cpp")])
    records, want = [], []
    for name, n in C.CASES:
        z, index = C.twin(name, n)[0], IC.own_index(name, n)
        records.append((z, index, n))
        want.append(IC.own_verdict(name, n)[1])
    for case in IC.FOREIGN:
        x, z, index = IC.foreign(*case)
        records.append((z, index, len(x)))
        want.append(IC.foreign_verdict(*case)[1])
    for (_, z, index, n), (_, res) in zip(IC.mutations(), IC.verdicts()):
        records.append((z, index, n))
        want.append(res)
    import deflate_ref
    records.append((deflate_ref.EMPTY, [], 0))
    want.append(I.inflate_indexed(deflate_ref.EMPTY, [], 0)[1])
    corpus = str(tmp_path/"corpus.bin")
    IC.write_corpus(corpus, records)
    run = subprocess.run([exe, corpus], capture_output=True, text=True, env={k: v for k, v in os.environ.items()
                                                                              if k != "LD_PRELOAD"})
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(want)
    keys = ("status", "bad_chunk", "adler32", "literals", "matches", "matched_bytes")
    for i, (line, res) in enumerate(zip(lines, want)):
        assert tuple(int(v) for v in line.split()) == tuple(res[k] for k in keys), (i, line, res)
    assert sum(1 for r in want if r["status"]) > 800
