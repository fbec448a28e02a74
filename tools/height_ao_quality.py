#!/usr/bin/env python3
"""What the height-map ambient occlusion (csrc/height_ao.hip) computes, against closed forms and
against its own finest setting; on the GPU through Context.height_ao, RGBA32F in and out.

  groove   H = s |x - 32| on 65 x 65, probed at its bottom, R = 32, cosine-weighted: the closed form is 1 / sqrt(1 + s^2)
  pit      a hemispherical pit of radius 24 in a plane, 65 x 65, probed at its bottom, R = 32: every horizon is the rim,
           one radius away and one radius up, so the cosine-weighted form is 1/2 and the uniform one 1 - 1/sqrt(2)
  photo    the luma of a 128 x 128 crop of a photograph (tests/golden/pvrtc_photos.npz, rgb[0]) as a height map of 16
           texels per unit, wrapped: D = 8 / 16 and R = 8 / 32 from the GPU against the numpy twin at D = 32, R = 64,
           as the PSNR of the occlusion (peak 1)

    python tools/height_ao_quality.py [--out profiles/height_ao_quality.md]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def rgba(h):
    img = np.zeros(h.shape + (4,), np.float32)
    img[..., 0] = h
    return img


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import height_ao_ref
    from cuttlefish_amd import Context
    lines = ["# Ambient occlusion from height maps: closed forms, and coarse settings against the finest", "",
             "`tools/height_ao_quality.py`, on the GPU (`Context.height_ao`, RGBA32F).", ""]
    x = np.arange(65)
    with Context(0) as ctx:
        lines += ["A V-groove `H = s|x - 32|` on 65 x 65 at its bottom, R = 32, cosine-weighted, against `1/sqrt(1+s^2)`:", "",
                  "| s | closed form | D = 8 | D = 16 | D = 32 |", "|---|---|---|---|---|"]
        for s in (0.5, 1.0, 2.0):
            h = np.tile((s*np.abs(x - 32)).astype(np.float32), (65, 1))
            got = [float(ctx.height_ao(rgba(h), 32, 1.0, D)[0][32, 32, 0]) for D in (8, 16, 32)]
            lines.append("| %g | %.6f | %s |" % (s, 1.0/math.sqrt(1.0 + s*s), " | ".join("%.6f" % v for v in got)))
        yy, xx = np.mgrid[0:65, 0:65] - 32
        r2 = (xx*xx + yy*yy).astype(np.float64)
        pit = np.where(r2 < 24.0**2, -np.sqrt(np.maximum(24.0**2 - r2, 0.0)), 0.0).astype(np.float32)
        lines += ["", "A hemispherical pit of radius 24 on 65 x 65 at its bottom, R = 32:", "",
                  "| visibility | closed form | D = 8 | D = 16 | D = 32 |", "|---|---|---|---|---|"]
        for name, uniform, closed in (("cosine-weighted", False, 0.5), ("uniform", True, 1.0 - 1.0/math.sqrt(2.0))):
            got = [float(ctx.height_ao(rgba(pit), 32, 1.0, D, uniform=uniform)[0][32, 32, 0]) for D in (8, 16, 32)]
            lines.append("| %s | %.6f | %s |" % (name, closed, " | ".join("%.6f" % v for v in got)))
        photo = np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"][0].astype(np.float64)
        luma = ((0.2126*photo[..., 0] + 0.7152*photo[..., 1] + 0.0722*photo[..., 2])/255.0).astype(np.float32)
        flags = height_ao_ref.WRAP_X | height_ao_ref.WRAP_Y
        best = height_ao_ref.occlusion(luma, 64, 16.0, 32, flags=flags)[0].astype(np.float32)
        lines += ["", "The luma of a photograph crop (128 x 128, 16 texels per unit, wrapped) against the twin at D = 32, "
                  "R = 64 (mean occlusion %.4f), PSNR of the occlusion in dB:" % float(best.mean()), "",
                  "| | R = 8 | R = 32 | R = 64 |", "|---|---|---|---|"]
        for D in (8, 16, 32):
            row = []
            for R in (8, 32, 64):
                got = ctx.height_ao(rgba(luma), R, 16.0, D, wrap=True)[0][..., 0]
                mse = float(np.mean((got.astype(np.float64) - best.astype(np.float64))**2))
                row.append("identical" if mse == 0.0 else "%.2f" % (10.0*math.log10(1.0/mse)))
            lines.append("| D = %d | %s |" % (D, " | ".join(row)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
