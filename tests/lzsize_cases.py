"""The payloads the deflate-size estimate is measured on (tests/test_lzsize_ref.py, tools/lzsize_quality.py): oracle
payloads at Quality.Normal of two inputs 1024 x 128 -- the six photo crops of tests/golden/pvrtc_photos.npz side by
side (repeated to 1024 texels) and synth.photo seed 1 -- for ten formats, and the BC1 / BC7 ones after rdo_ref.rdo."""
import functools
import os

import numpy as np

import oracle_lib
import rdo_ref
from cuttlefish_amd import Format, Type, synth

HERE = os.path.dirname(os.path.abspath(__file__))

FORMATS = (("BC1", Format.BC1_RGB, Type.UNorm), ("BC3", Format.BC3, Type.UNorm), ("BC5", Format.BC5, Type.UNorm),
           ("BC7", Format.BC7, Type.UNorm), ("BC6H UFloat", Format.BC6H, Type.UFloat),
           ("ETC2 RGB", Format.ETC2_R8G8B8, Type.UNorm), ("ETC2 RGBA8", Format.ETC2_R8G8B8A8, Type.UNorm),
           ("ASTC 4x4", Format.ASTC_4x4, Type.UNorm), ("ASTC 6x6", Format.ASTC_6x6, Type.UNorm),
           ("ASTC 8x8", Format.ASTC_8x8, Type.UNorm))
RDO_LAMBDAS = {"BC1": (2.0, 8.0, 32.0), "BC7": (1.0, 4.0, 16.0)}
TARGET_PAIRS = [(inp, fmt) for inp in ("crops", "photo") for fmt in ("BC1", "BC7")]


@functools.lru_cache(maxsize=None)
def inputs():
    crops = [np.ascontiguousarray(c) for c in np.load(os.path.join(HERE, "golden", "pvrtc_photos.npz"))["rgb"]]
    return {"crops": np.ascontiguousarray(np.concatenate(crops + crops, axis=1)[:, :1024]),
            "photo": synth.photo(1024, 128, seed=1)}


@functools.lru_cache(maxsize=None)
def plain(inp: str, name: str) -> np.ndarray:
    _, fmt, typ = next(f for f in FORMATS if f[0] == name)
    return oracle_lib.encode(inputs()[inp], int(fmt), int(typ), 2)


def format_of(name: str):
    return next((int(f), int(t)) for n, f, t in FORMATS if n == name)


def payload_rows():
    """[(row name, payload)]: every format plain, then BC1 / BC7 after the pass"""
    rows = []
    for inp in inputs():
        for name, _, _ in FORMATS:
            rows.append(("%s %s" % (inp, name), plain(inp, name)))
        for name, lams in RDO_LAMBDAS.items():
            fmt, typ = format_of(name)
            for lam in lams:
                out, _ = rdo_ref.rdo(plain(inp, name), inputs()[inp], fmt, typ, lam)
                rows.append(("%s %s rdo %g" % (inp, name, lam), out))
    return rows


def flat_and_ramp():
    """the rows that are reported, not asserted: a flat image and a ramp, as BC1 and BC7"""
    flat = np.full((128, 1024, 4), 200, np.uint8)
    ramp = np.zeros((128, 1024, 4), np.uint8)
    ramp[..., :3] = (np.arange(1024)//4)[None, :, None]
    ramp[..., 3] = 255
    rows = []
    for what, img in (("flat", flat), ("ramp", ramp)):
        for name in ("BC1", "BC7"):
            fmt, typ = format_of(name)
            rows.append(("%s %s" % (what, name), oracle_lib.encode(img, fmt, typ, 2)))
    return rows
