"""The host part of the texel vocabulary (csrc/cf_texel.h) on the CPU: tools/texel_host.cpp, built from the header with a
host compiler alone -- once plain, once with -fsanitize=address,undefined -- against numpy, exhaustively where that is
cheap.  The header needs _Float16, so the compiler is ROCm's host clang++.  The sanitised program runs as a child process
of its own; nothing is preloaded into it."""
import os
import subprocess

import numpy as np
import pytest

from cuttlefish_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL_BYTES = {0: 4, 1: 16, 2: 8}                  # CFHIP_PIXEL_RGBA8, _RGBA32F, _RGBA16F
SIDES = (1, 2, 3, 64, 65)
INT32_MIN = -2**31


@pytest.fixture(scope="module", params=[(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "sanitised"])
def exe(request, tmp_path_factory):
    cxx = os.path.join(build.LLVM_BIN, "clang++")
    if not os.path.exists(cxx):
        pytest.fail("no ROCm host clang++ under %s" % build.LLVM_BIN)
    path = str(tmp_path_factory.mktemp("texel")/"texel_host")
    # -ffp-contract=off as the library is built: v*255.0 + 0.5 is a product and a sum
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", *request.param, "-o", path,
                           os.path.join(ROOT, "tools", "texel_host.cpp")])
    return path


def _run(exe, *args, data=b""):
    run = subprocess.run([exe, *args], input=data, capture_output=True,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert run.returncode == 0 and run.stderr == b"", run.stderr.decode()
    return run.stdout


def _around(values, dtype):
    """every value and its neighbour one ulp either side"""
    v = np.asarray(values, dtype)
    return np.concatenate([v, np.nextafter(v, dtype(-np.inf)), np.nextafter(v, dtype(np.inf))])


def test_decode_of_every_byte_and_every_half(exe):
    got = np.frombuffer(_run(exe, "decode"), np.uint32)
    assert got.size == 256 + 65536
    u8 = (np.arange(256, dtype=np.float64)/255.0).astype(np.float32)
    assert np.array_equal(got[:256], u8.view(np.uint32))
    # every bit pattern, NaN payloads included
    half = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(got[256:], half.view(np.uint32))


def test_unit_value_to_8_bits(exe):
    v = _around(np.arange(511, dtype=np.float64)/510.0, np.float64)
    got = np.frombuffer(_run(exe, "unit_u8", data=v.tobytes()), np.uint8)
    assert np.array_equal(got, np.floor(v*255.0 + 0.5).astype(np.uint8))
    # k/510 are the 256 codes and the 255 ties between them: a tie goes up
    assert np.array_equal(got[:511], (np.arange(511) + 1)//2)


def test_float_to_half_is_nearest_even(exe):
    halves = np.arange(0x3C00 + 1, dtype=np.uint16).view(np.float16).astype(np.float32)     # [0, 1], in order
    ties = (halves[:-1].astype(np.float64) + halves[1:].astype(np.float64))/2.0
    assert np.array_equal(ties.astype(np.float32).astype(np.float64), ties)                # floats, exactly
    v = _around(np.concatenate([halves, ties.astype(np.float32)]), np.float32)
    got = np.frombuffer(_run(exe, "to_half", data=v.tobytes()), np.uint16)
    assert np.array_equal(got, v.astype(np.float16).view(np.uint16))
    # a half comes back as itself, a tie goes to the even neighbour
    n = halves.size
    assert np.array_equal(got[:n], np.arange(n))
    lower = np.arange(n - 1)
    assert np.array_equal(got[n:2*n - 1], lower + (lower & 1))


def test_pixel_size_and_coordinates(exe):
    lines = _run(exe, "coords", *[str(s) for s in SIDES]).decode().splitlines()
    sizes = [line.split() for line in lines if line.startswith("size")]
    assert {int(t): int(b) for _, t, b in sizes} == PIXEL_BYTES
    rows = [[int(v) for v in line.split()] for line in lines if not line.startswith("size")]
    want = [(side, at) for side in SIDES for at in range(-3*side, 3*side + 1)] + [(1, INT32_MIN + 1)]
    assert [(r[0], r[1]) for r in rows] == want
    for side, at, mod, there, there_wrapped, wrapped in rows:
        assert mod == at % side and wrapped == at % side, (side, at)          # Python's % is the floor modulo
        assert there == (0 <= at < side) and there_wrapped == 1, (side, at)
