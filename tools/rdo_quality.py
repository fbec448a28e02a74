#!/usr/bin/env python3
"""profiles/rdo_quality.md: what the rate-distortion pass buys and costs, measured on the
CPU with its definition, tests/rdo_ref.py, on payloads of the CPU oracle at Quality.Normal.

Inputs: the six 128^2 photo crops of tests/golden/pvrtc_photos.npz and synth.photo 512^2 (seed 1).  Per format of
the table and lambda in {1, 2, 4, 8, 16}: the deflate-9 size of the optimised payload over the plain one (pooled
over the crops: summed sizes; and the range over the crops) and the PSNR lost over the compared channels; the same
with max_sse_increase at two settings.  A last table measures the segment length: whole rows against segments of
64 / 128 / 256 blocks on inputs 256 blocks wide.

    python tools/rdo_quality.py > profiles/rdo_quality.md
"""
import math
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import oracle_lib  # noqa: E402
import rdo_ref  # noqa: E402
from cuttlefish_amd import Format, synth  # noqa: E402

LAMBDAS = (1, 2, 4, 8, 16)
CAPS = (None, 256, 64)


def deflated(p):
    return len(zlib.compress(np.asarray(p).tobytes(), 9))


def psnr(sse, texels, channels):
    return float("inf") if sse == 0 else 10.0*math.log10(255.0*255.0*texels*channels/sse)


def measure(fmt, images, plain, lam, cap):
    """(pooled ratio, min ratio, max ratio, min PSNR loss, max PSNR loss) over the images"""
    ratios, losses, a, b = [], [], 0, 0
    nch = len(rdo_ref.TABLE[(fmt, 0)][1])
    for im, p in zip(images, plain):
        out, st = rdo_ref.rdo(p, im, fmt, 0, lam, max_sse_increase=cap)
        x, y = deflated(out), deflated(p)
        a, b = a + x, b + y
        ratios.append(x/y)
        tex = im.shape[0]*im.shape[1]
        losses.append(psnr(st["sse_before"], tex, nch) - psnr(st["sse_after"], tex, nch))
    return a/b, min(ratios), max(ratios), min(losses), max(losses)


def main():
    crops = [np.ascontiguousarray(c) for c in np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]]
    photo = [synth.photo(512, 512, seed=1)]
    print("# Rate-distortion pass: deflate-9 size and PSNR loss (CPU twin, oracle payloads, Quality.Normal)\n")
    print("Produced by `tools/rdo_quality.py`.  ratio = deflate-9 size of the optimised payload / of the plain one;")
    print("pooled = summed over the six crops.  PSNR loss in dB over the channels the format stores.  cap =")
    print("`max_sse_increase` per block.  L = %d, SEG = %d.\n" % (rdo_ref.L, rdo_ref.SEG))
    for fmt, typ in sorted(rdo_ref.TABLE):
        plain_c = [oracle_lib.encode(c, fmt, typ, 2) for c in crops]
        plain_p = [oracle_lib.encode(c, fmt, typ, 2) for c in photo]
        print("## %s\n" % Format(fmt).name)
        print("| lambda | cap | crops pooled | per crop | PSNR loss per crop | photo 512^2 | its PSNR loss |")
        print("|---|---|---|---|---|---|---|")
        for cap in CAPS:
            for lam in LAMBDAS:
                c = measure(fmt, crops, plain_c, lam, cap)
                p = measure(fmt, photo, plain_p, lam, cap)
                print("| %d | %s | %.3f | %.3f – %.3f | %.2f – %.2f | %.3f | %.2f |" % (
                    lam, "none" if cap is None else cap, c[0], c[1], c[2], c[3], c[4], p[0], p[4]), flush=True)
        print()
    print("## Segment length\n")
    print("Inputs 256 blocks wide: synth.photo 1024 x 256 (seed 1), synth.photo2 1024 x 256, and the six crops side")
    print("by side twice (1536 x 128 is 384 blocks; cut to 1024).  ratio as above; `rows` = unsegmented block rows.\n")
    print("| format | lambda | input | rows | SEG 256 | SEG 128 | SEG 64 |")
    print("|---|---|---|---|---|---|---|")
    wide = {"photo": synth.photo(1024, 256, seed=1), "photo2": synth.photo2(1024, 256),
            "crops": np.ascontiguousarray(np.concatenate(crops + crops, axis=1)[:, :1024])}
    pooled = {}
    for fmt, lam in ((rdo_ref.BC1_RGB, 3), (rdo_ref.BC3, 3), (rdo_ref.BC7, 3)):
        for name, im in wide.items():
            p = oracle_lib.encode(im, fmt, 0, 2)
            base = deflated(p)
            sizes = [deflated(rdo_ref.rdo(p, im, fmt, 0, lam, seg=s)[0]) for s in (0, 256, 128, 64)]
            print("| %s | %d | %s | %s |" % (Format(fmt).name, lam, name, " | ".join("%.4f" % (s/base) for s in sizes)),
                  flush=True)
            acc = pooled.setdefault(fmt, [0]*5)
            for k, s in enumerate(sizes + [base]):
                acc[k] += s
    for fmt, acc in pooled.items():
        print("| %s | 3 | pooled | %s |" % (Format(fmt).name, " | ".join("%.4f" % (s/acc[4]) for s in acc[:4])))


if __name__ == "__main__":
    main()
