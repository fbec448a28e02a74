"""The stage log's pair-to-stage mapping and validity rule (csrc/stage_log.h) on the CPU: tools/stage_log_host.cpp, built
with the host compiler alone -- once plain, once with -fsanitize=address,undefined -- against the three formulas the six
cfhip_*_stage_ms functions spelled out one by one before they shared the header.  The sanitised program runs as a child
process of its own; nothing is preloaded into it."""
import os
import shutil
import subprocess

import pytest

from cuttlefish_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DF = len(api.DEFLATE_STAGES)
# family: (head, per_slice, tail), as cfhip_api.hip opens the log
GEOMETRY = {"lz_size": (0, len(api.LZ_STAGES), 0), "deflate": (0, DF, 0), "inflate": (0, len(api.INFLATE_STAGES), 0),
            "lz4_encode": (0, len(api.LZ4_ENCODE_STAGES) - 1, 1), "lz4_decode": (len(api.LZ4_DECODE_STAGES), 0, 0),
            "png_encode": (1, DF, 2)}
SLICES = (1, 2, 3)


def _old_modulo(i, pairs, stages):
    """cfhip_lz_stage_ms, cfhip_deflate_stage_ms, cfhip_inflate_stage_ms: ms[i % S]"""
    return i % stages


def _old_lz4(i, pairs, per, stages):
    """lz4_stage_ms: a slice's `per` stages repeat, the rest follow once"""
    tail = stages - per
    return i % per if i < pairs - tail else per + (i - (pairs - tail))


def _old_png(i, pairs):
    """cfhip_png_stage_ms: the first pair is the filter's, the last two are crc and final, the encoder's slices between"""
    return 0 if i == 0 else len(api.PNG_STAGES) - (pairs - i) if i >= pairs - 2 else 1 + (i - 1) % DF


OLD = {"lz_size": lambda i, n: _old_modulo(i, n, len(api.LZ_STAGES)),
       "deflate": lambda i, n: _old_modulo(i, n, DF),
       "inflate": lambda i, n: _old_modulo(i, n, len(api.INFLATE_STAGES)),
       "lz4_encode": lambda i, n: _old_lz4(i, n, len(api.LZ4_ENCODE_STAGES) - 1, len(api.LZ4_ENCODE_STAGES)),
       # the decoder called the same routine with per_slice = stages: one "slice", no tail
       "lz4_decode": lambda i, n: _old_lz4(i, n, len(api.LZ4_DECODE_STAGES), len(api.LZ4_DECODE_STAGES)),
       "png_encode": _old_png}


def _pairs(family, slices):
    head, per, tail = GEOMETRY[family]
    return head + slices*per + tail


@pytest.fixture(scope="module", params=[(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "sanitised"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    path = str(tmp_path_factory.mktemp("stage_log")/"stage_log_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *request.param, "-o", path,
                           os.path.join(ROOT, "tools", "stage_log_host.cpp")])
    return path


def _run(exe, cases):
    """cases: (family, first, pairs, events_used) -> per case None (not valid) or the stage of every pair"""
    args = [str(v) for family, first, pairs, used in cases for v in (*GEOMETRY[family], first, pairs, used)]
    run = subprocess.run([exe, *args], capture_output=True, text=True,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(lines) == len(cases)
    return [line[1:] if line[0] else None for line in lines]


def test_stage_tuples_match_the_geometries():
    for family, names in (("lz_size", api.LZ_STAGES), ("deflate", api.DEFLATE_STAGES), ("inflate", api.INFLATE_STAGES),
                          ("lz4_encode", api.LZ4_ENCODE_STAGES), ("lz4_decode", api.LZ4_DECODE_STAGES),
                          ("png_encode", api.PNG_STAGES)):
        assert sum(GEOMETRY[family]) == len(names), family


def test_mapping_equals_the_old_formulas(exe):
    # the decoder has no slices: its one pair count, whatever the input's size
    cases = [(f, first, _pairs(f, 0 if f == "lz4_decode" else s), first + 2*_pairs(f, s) + slack)
             for f in GEOMETRY for s in SLICES for first, slack in ((0, 0), (6, 4))]
    for (family, first, pairs, used), got in zip(cases, _run(exe, cases)):
        assert got == [OLD[family](i, pairs) for i in range(pairs)], (family, pairs)
        # every stage is timed, a slice's stages once per slice
        assert sorted(set(got)) == list(range(sum(GEOMETRY[family]))), (family, pairs)


def test_invalid_logs_are_rejected(exe):
    big = 1000
    cases, why = [], []
    for family, (head, per, tail) in GEOMETRY.items():
        cases.append((family, 0, 0, big))
        why.append("no pairs")
        for s in SLICES:
            good = _pairs(family, 0 if family == "lz4_decode" else s)
            for pairs in (good - 1, good + 1):
                if pairs > 0:
                    cases.append((family, 0, pairs, big))
                    why.append("not head + k*per_slice + tail")
            # the events were given to a later call: fewer in use than the log's last pair
            cases.append((family, 2, good, 2 + 2*good - 1))
            why.append("pairs beyond the events in use")
    # the PNG writer without one whole slice of its encoder: cfhip_png_stage_ms's pairs < 3 + CFDF_STAGES
    for pairs in range(3 + DF):
        cases.append(("png_encode", 0, pairs, big))
        why.append("pairs < 3 + CFDF_STAGES")
    # head and tail alone are no call of a family that has slices
    cases.append(("lz4_encode", 0, 1, big))
    why.append("tail alone")
    for case, reason, got in zip(cases, why, _run(exe, cases)):
        assert got is None, (case, reason)
