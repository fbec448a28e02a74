#!/usr/bin/env python3
"""profiles/rdo_quality.md: what the rate-distortion pass buys and costs, measured on the
CPU with its definition, tests/rdo_ref.py, on payloads of the CPU oracle at Quality.Normal.

Inputs: the six 128^2 photo crops of tests/golden/pvrtc_photos.npz and synth.photo 512^2 (seed 1).  Per format of
the table and lambda in {1, 2, 4, 8, 16}: the deflate-9 size of the optimised payload over the plain one (pooled
over the crops: summed sizes; and the range over the crops) and the PSNR lost over the compared channels; the same
with max_sse_increase at two settings.  A last table measures the segment length: whole rows against segments of
64 / 128 / 256 blocks on inputs 256 blocks wide.

    python tools/rdo_quality.py > profiles/rdo_quality.md

With --row-above it writes profiles/rdo2d_quality.md instead: the pass with copies from the block row above
(tests/rdo2d_ref.py) beside the plain one, on the six crops and on the three inputs 256 blocks wide of the last
table, per format and lambda; for BC1 / BC3 / BC7 the PSNR lost at the same size; and the tile height and the
number of positions above on BC1 and BC7.  The runs are spread over --jobs processes.

    python tools/rdo_quality.py --row-above > profiles/rdo2d_quality.md
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
import rdo2d_ref  # noqa: E402
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


def inputs2d():
    """{name: [images]}: the six crops, and the three inputs 256 blocks wide"""
    crops = [np.ascontiguousarray(c) for c in np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]]
    return {"crops": crops, "photo": [synth.photo(1024, 256, seed=1)], "photo2": [synth.photo2(1024, 256)],
            "crops wide": [np.ascontiguousarray(np.concatenate(crops + crops, axis=1)[:, :1024])]}


_INPUTS, _PLAIN = None, {}


def run2d(task):
    """(fmt, input, lambda, variant) -> its key and (deflate-9 bytes, sse after, sse before) summed over the input's
    images; variant None is the payload as encoded, else the keywords of rdo2d_ref.rdo2d"""
    global _INPUTS
    fmt, name, lam, variant = task
    if _INPUTS is None:
        _INPUTS = inputs2d()
    images = _INPUTS[name]
    if (fmt, name) not in _PLAIN:
        _PLAIN[(fmt, name)] = [oracle_lib.encode(im, fmt, 0, 2) for im in images]
    size = after = before = 0
    for im, p in zip(images, _PLAIN[(fmt, name)]):
        if variant is None:
            size += deflated(p)
            continue
        out, st = rdo2d_ref.rdo2d(p, im, fmt, 0, lam, None, (True,)*4, **variant)
        size, after, before = size + deflated(out), after + st["sse_after"], before + st["sse_before"]
    return (fmt, name, lam, repr(variant)), (size, after, before)


def interpolate(x, xs, ys):
    """ys at x on the polyline (xs, ys), xs falling; None outside it"""
    for (x0, y0), (x1, y1) in zip(zip(xs, ys), zip(xs[1:], ys[1:])):
        if x1 <= x <= x0:
            return y0 if x0 == x1 else y0 + (y1 - y0)*(x0 - x)/(x0 - x1)
    return None


def main2d(jobs):
    from concurrent.futures import ProcessPoolExecutor
    names = ("crops", "photo", "photo2", "crops wide")
    plain_v, above_v = dict(row_above=False), dict(row_above=True)
    fmts = [f for f, _ in sorted(rdo_ref.TABLE)]
    tiles = [dict(row_above=True, tile_rows=r) for r in (4, 8, 16, 64)] + [dict(row_above=True, up=16)]
    study = ((rdo_ref.BC1_RGB, 4), (rdo_ref.BC7, 2))
    tasks = [(f, n, 0, None) for f in fmts for n in names]
    tasks += [(f, n, lam, v) for f in fmts for n in names for lam in LAMBDAS for v in (plain_v, above_v)]
    tasks += [(f, n, lam, v) for f, lam in study for n in names for v in tiles]
    with ProcessPoolExecutor(jobs) as ex:
        res = dict(ex.map(run2d, tasks, chunksize=4))
    texels = {n: sum(im.shape[0]*im.shape[1] for im in ims) for n, ims in inputs2d().items()}

    def point(f, n, lam, v):
        """(ratio, PSNR loss)"""
        size, after, before = res[(f, n, lam, repr(v))]
        nch = len(rdo_ref.TABLE[(f, 0)][1])
        return size/res[(f, n, 0, repr(None))][0], psnr(before, texels[n], nch) - psnr(after, texels[n], nch)

    print("# Rate-distortion pass with copies from the block row above (CPU twin, oracle payloads, Quality.Normal)\n")
    print("Produced by `tools/rdo_quality.py --row-above`.  Every entry is ratio / PSNR loss: the deflate-9 size of the")
    print("optimised payload over the plain one, and the dB lost over the channels the format stores.  `left` is the")
    print("pass of profiles/rdo_quality.md, `+above` the same with the row above (tests/rdo2d_ref.py; TILE_ROWS = %d," % rdo2d_ref.TILE_ROWS)
    print("UP = %d, L = %d, SEG = %d).  crops: the six 128^2 photo crops, sizes and errors summed; photo, photo2:" % (
        rdo2d_ref.UP, rdo_ref.L, rdo_ref.SEG))
    print("synth.photo (seed 1) and synth.photo2 at 1024 x 256; crops wide: the crops side by side, 1024 x 128.\n")
    for f in fmts:
        print("## %s\n" % Format(f).name)
        print("| lambda | " + " | ".join("%s left | %s +above" % (n, n) for n in names) + " |")
        print("|---|" + "---|"*(2*len(names)))
        for lam in LAMBDAS:
            cells = ["%.3f / %.2f" % point(f, n, lam, v) for n in names for v in (plain_v, above_v)]
            print("| %d | %s |" % (lam, " | ".join(cells)))
        print()
    print("## PSNR loss at the same size\n")
    print("For each lambda of the pass with the row above: its ratio and loss, and the loss of the left-only pass at that")
    print("ratio (its lambda interpolated on its own curve through lambda = 1 .. 16; `-` where the ratio lies outside")
    print("that curve).\n")
    print("| format | input | lambda | ratio | loss +above | loss left at that ratio |")
    print("|---|---|---|---|---|---|")
    for f in (rdo_ref.BC1_RGB, rdo_ref.BC3, rdo_ref.BC7):
        for n in ("crops", "crops wide", "photo"):
            curve = [point(f, n, lam, plain_v) for lam in LAMBDAS]
            for lam in LAMBDAS:
                ratio, loss = point(f, n, lam, above_v)
                at = interpolate(ratio, [c[0] for c in curve], [c[1] for c in curve])
                print("| %s | %s | %d | %.3f | %.2f | %s |" % (Format(f).name, n, lam, ratio, loss,
                                                           "-" if at is None else "%.2f" % at))
    print("\n## Tile height and positions above\n")
    print("| format | lambda | input | left | TILE_ROWS 4 | 8 | 16 | 64 | 8 rows, UP 16 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for f, lam in study:
        for n in names:
            cells = ["%.4f / %.2f" % point(f, n, lam, v) for v in [plain_v] + tiles]
            print("| %s | %d | %s | %s |" % (Format(f).name, lam, n, " | ".join(cells)))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--row-above", action="store_true", help="write profiles/rdo2d_quality.md's content instead")
    ap.add_argument("--jobs", type=int, default=6)
    args = ap.parse_args()
    main2d(args.jobs) if args.row_above else main()
