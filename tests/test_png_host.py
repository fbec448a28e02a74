"""The logic the PNG kernels share with the host (csrc/png.h) on the CPU: tools/png_host.cpp, built with the host compiler
alone -- once plain, once with -fsanitize=address,undefined -- against the definition, tests/png_ref.py.  It filters and
assembles files from raw texels (the IDAT body a stored zlib stream), which the twin's reader and Pillow open to the
twin's samples, row types and filtered bytes; and it reads the twin's files back, taking the IDAT CRC from pieces the way
the kernels do.  The sanitised program runs as a child process of its own; nothing is preloaded into it."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL_TYPE = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.float16): 2}
# every colour type x depth x source type at the odd sizes, and one image of several CRC pieces (more than 16 KiB)
CASES = [(w, h, dt, ct, d) for w, h in ((1, 1), (7, 1), (5, 3), (67, 29)) for dt in P.DTYPES for ct in P.COLOR_TYPES
         for d in P.DEPTHS] + [(300, 40, np.float32, P.RGBA, 16), (64, 10, np.uint8, P.GREY, 8)]


def _image(w, h, dt, ct):
    if (w, h, ct) == (64, 10, P.GREY):
        return P.five_filter_image()
    return P.image(w, h, dt)


@pytest.fixture(scope="module", params=[(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "sanitised"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    path = str(tmp_path_factory.mktemp("png")/"png_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", *request.param, "-o", path,
                           os.path.join(ROOT, "tools", "png_host.cpp"), "-lz"])
    return path


def _run(exe, *args):
    run = subprocess.run([exe, *args], capture_output=True, text=True,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert run.returncode == 0 and run.stderr == "", run.stderr
    return [int(v) for v in run.stdout.split()]


def test_host_program_writes_what_the_twin_defines(exe, tmp_path):
    for i, (w, h, dt, ct, depth) in enumerate(CASES):
        img = _image(w, h, dt, ct)
        srgb = i % 2
        # a pitch wider than tight: the texels of one more pixel per row, never read
        wide = np.zeros((h, w + 1, 4), img.dtype)
        wide[:, :w] = img
        src, out = str(tmp_path/"image.bin"), str(tmp_path/"out.png")
        with open(src, "wb") as f:
            f.write(struct.pack("<7I", w, h, PIXEL_TYPE[img.dtype], wide.strides[0], ct, depth, srgb))
            f.write(wide.tobytes())
        line = _run(exe, "encode", src, out)
        data = open(out, "rb").read()
        want_bytes, want_rows = P.filtered(img, ct, depth)
        assert line[:5] == want_rows and line[6] == zlib.crc32(want_bytes), (w, h, dt, ct, depth)
        chunks = P.read_chunks(data)                                  # every CRC, the IDAT one from pieces
        assert zlib.decompress(chunks[-2][1]) == want_bytes and line[5] == zlib.crc32(b"IDAT" + chunks[-2][1])
        samples, d, c, s, types = P.read(data)
        assert (d, c, s) == (depth, ct, bool(srgb))
        assert np.array_equal(samples, P.quantise(img, depth)[..., list(P.CHANNELS[ct])])
        assert len(data) <= P.png_bound(w, h, ct, depth, srgb)
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h)


def test_host_program_reads_the_twins_files(exe, tmp_path):
    for i, (w, h, dt, ct, depth) in enumerate(CASES):
        img = _image(w, h, dt, ct)
        data, res = P.encode(img, ct, depth, bool(i % 2))
        src, out = str(tmp_path/"twin.png"), str(tmp_path/"rows.raw")
        with open(src, "wb") as f:
            f.write(data)
        line = _run(exe, "read", src, out)
        assert line[:5] == [w, h, depth, ct, i % 2]
        assert [line[5:].count(t) for t in range(5)] == res["rows_by_filter"]
        assert open(out, "rb").read() == P.raw_rows(img, ct, depth).tobytes()
    # a damaged file is refused: one bit of the IDAT data
    bad = bytearray(data)
    bad[60] ^= 4
    with open(src, "wb") as f:
        f.write(bytes(bad))
    run = subprocess.run([exe, "read", src, out], capture_output=True, text=True,
                         env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert run.returncode == 1 and "CRC" in run.stderr
