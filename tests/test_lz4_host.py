"""The decode logic the kernels run (csrc/lz4.h) on the CPU: tools/lz4_host.cpp, built with the host compiler alone --
once plain, once with -fsanitize=address,undefined -- on the whole corpus: the twin's frames, liblz4's frames of the
fixture and every mutation, against the definition, tests/lz4_ref.py, record by record.  The sanitised program runs as a
child process of its own; nothing is preloaded into it."""
import collections
import os
import shutil
import subprocess

import pytest

import lz4_cases as LC
import lz4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [(c, n) for c, n in LC.CASES if n <= 65537] + [("zeros", 200*1024), ("text", 200*1024)]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """-> (the corpus file, the line the twin expects per record)"""
    records, want = [], []

    def add(z, n, out, res):
        records.append((z, n))
        ok = res["status"] == 0
        want.append((res["status"], res["bad_block"], R.xxh32(out) if ok else 0, res["blocks_compressed"],
                     res["blocks_stored"], res["sequences"], res["literals"], res["matched_bytes"],
                     res["content_checksum"]))
    for name, n in HOST_CASES:
        z = LC.twin(name, n)[0]
        add(z, n, *R.decode(z, n))
    for w, i in LC.FOREIGN_ALL:
        x, z = LC.foreign(w, i)
        add(z, len(x), *R.decode(z, len(x)))
    for key in ("linked", "big"):
        add(LC.fixture()[key], 200*1024, *R.decode(LC.fixture()[key], 200*1024))
    for (_, z, n), (out, res) in zip(LC.mutations(), LC.verdicts()):
        add(z, n, out, res)
    add(R.EMPTY, 0, *R.decode(R.EMPTY, 0))
    path = str(tmp_path_factory.mktemp("lz4")/"corpus.bin")
    LC.write_corpus(path, records)
    return path, want


def test_corpus_reaches_every_class(corpus):
    _, want = corpus
    failing = collections.Counter(w[0] for w in want if w[0])
    print("failing records per class:", {R.CLASSES[k]: v for k, v in sorted(failing.items())})
    assert sum(failing.values()) >= 500
    for status in range(1, 8):
        assert failing[status] >= 5, (R.CLASSES[status], failing)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitised"])
def test_host_program_matches_the_twin(tmp_path, corpus, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path/"lz4_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe,
                           os.path.join(ROOT, "tools", "lz4_host.cpp")])
    path, want = corpus
    run = subprocess.run([exe, path], capture_output=True, text=True,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(want)
    for i, (line, w) in enumerate(zip(lines, want)):
        assert tuple(int(v) for v in line.split()) == w, (i, line, w)
