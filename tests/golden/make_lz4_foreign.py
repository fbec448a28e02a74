"""Writes tests/golden/lz4_foreign.npz: LZ4 frames made by liblz4's LZ4F_compressFrame (through ctypes), so that the
GPU tests read an independent encoder's frames without needing the library.

  set A   64 KiB independent blocks, block checksums off, content size off, content checksum on
  set B   64 KiB independent blocks, block checksums on, content size on, content checksum off
  rejected: `linked` (64 KiB linked blocks) and `big` (256 KiB independent blocks), both of zeros-204800

over the inputs of tests/lz4_cases.py FOREIGN (text 20000, BC1 rdo 32768, BC7 65537, zeros 204800, random 65537).  The
file holds the frames only; the inputs are lz4_cases.content(name, n).

    python tests/golden/make_lz4_foreign.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint*3)]


def compress_frame(lib, data: bytes, block_id=4, independent=1, content_checksum=0, content_size=0, block_checksum=0):
    prefs = Preferences()
    prefs.frameInfo.blockSizeID, prefs.frameInfo.blockMode = block_id, independent
    prefs.frameInfo.contentChecksumFlag, prefs.frameInfo.blockChecksumFlag = content_checksum, block_checksum
    prefs.frameInfo.contentSize = len(data) if content_size else 0
    lib.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    lib.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    lib.LZ4F_compressFrame.restype = ctypes.c_size_t
    lib.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.LZ4F_isError.argtypes = [ctypes.c_size_t]
    cap = lib.LZ4F_compressFrameBound(len(data), ctypes.byref(prefs))
    out = ctypes.create_string_buffer(cap)
    n = lib.LZ4F_compressFrame(out, cap, data, len(data), ctypes.byref(prefs))
    assert not lib.LZ4F_isError(n), n
    return out.raw[:n]


def main():
    import lz4_cases as LC
    lib = ctypes.CDLL("liblz4.so.1")
    arrays = {}
    for i, (name, n) in enumerate(LC.FOREIGN):
        data = LC.content(name, n).tobytes()
        arrays["a%d" % i] = np.frombuffer(compress_frame(lib, data, content_checksum=1), np.uint8)
        arrays["b%d" % i] = np.frombuffer(compress_frame(lib, data, content_size=1, block_checksum=1), np.uint8)
    zeros = LC.content("zeros", 200*1024).tobytes()
    arrays["linked"] = np.frombuffer(compress_frame(lib, zeros, independent=0), np.uint8)
    arrays["big"] = np.frombuffer(compress_frame(lib, zeros, block_id=5), np.uint8)
    path = os.path.join(HERE, "lz4_foreign.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 512*1024
    # the twin's verdict on every mutation of tests/lz4_cases.py, for the GPU test (tests/test_lz4_ref.py holds it to the twin)
    import json
    LC.fixture.cache_clear()
    rows = [[label, res["status"], res["bad_block"]] for (label, _, _), (_, res) in zip(LC.mutations(), LC.verdicts())]
    with open(os.path.join(HERE, "lz4_mutations.json"), "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
