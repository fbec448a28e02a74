"""PVRTC1 4 bpp on one GPU: one JSON line per (format, level, size) at 2048^2 and 4096^2 -- summed kernel ms
(cfhip_profile_begin / end), launches, Mpixel/s, PSNR on the tests/golden/pvrtc_photos.npz crops and on
synth.photo -- then decode and decode + SSE ms at 8192^2, and BC1 Normal's PSNR on the same crops for context.

Run from the repository root: python tools/bench_pvrtc.py [--reps N] [--sizes 2048,4096]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth  # noqa: E402

FIX = os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz")


def psnr(sse, n, ch):
    return api.psnr_from_sse(sse, n, ch)


def crops_psnr(ctx, fmt, q):
    z = np.load(FIX)
    imgs = list(z["rgb"]) if fmt == Format.PVRTC1_RGB_4BPP else list(z["rgba"])
    ch = 3 if fmt == Format.PVRTC1_RGB_4BPP else 4
    outs = ctx.encode_pvrtc(imgs, make_params(fmt, Type.UNorm, q))
    sse = [sum(v) for v in zip(*[ctx.decode_pvrtc_sse(o, im, fmt)[:ch] for o, im in zip(outs, imgs)])]
    return psnr(sse, sum(im.shape[0] * im.shape[1] for im in imgs), ch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="2048,4096")
    a = ap.parse_args()
    with Context(0) as ctx:
        for size in [int(s) for s in a.sizes.split(",")]:
            img = synth.photo(size, size, seed=1)
            for fmt in (Format.PVRTC1_RGB_4BPP, Format.PVRTC1_RGBA_4BPP):
                ch = 3 if fmt == Format.PVRTC1_RGB_4BPP else 4
                for q in Quality:
                    p = make_params(fmt, Type.UNorm, q)
                    ctx.encode_pvrtc([img], p)                      # warm-up
                    best, launches, out = None, 0, None
                    for _ in range(a.reps):
                        ctx.profile_begin()
                        out = ctx.encode_pvrtc([img], p)[0]
                        ms, launches = ctx.profile_end()
                        best = ms if best is None else min(best, ms)
                    print(json.dumps({"format": fmt.name, "quality": q.name, "size": size, "kernel_ms": round(best, 3),
                                      "launches": launches, "mpix_s": round(size * size / best / 1e3, 1),
                                      "psnr_synth": round(psnr(ctx.decode_pvrtc_sse(out, img, fmt)[:ch], size * size, ch), 3),
                                      "psnr_crops": round(crops_psnr(ctx, fmt, q), 3)}), flush=True)
        big = 8192
        rng = np.random.default_rng(0)
        payload = rng.integers(0, 256, api.pvrtc_payload_size(Format.PVRTC1_RGBA_4BPP, Type.UNorm, big, big), np.uint8)
        ref = np.zeros((big, big, 4), np.uint8)
        for name, call in (("decode", lambda: ctx.decode_pvrtc(payload, Format.PVRTC1_RGBA_4BPP, big, big)),
                           ("decode_sse", lambda: ctx.decode_pvrtc_sse(payload, ref, Format.PVRTC1_RGBA_4BPP))):
            call()
            ms = min((call(), ctx.last_kernel_ms())[1] for _ in range(a.reps))
            print(json.dumps({"op": name, "size": big, "kernel_ms": round(ms, 3),
                              # payload read + 4 bytes per texel (written by decode, read by decode_sse)
                              "gb_s": round((payload.nbytes + big * big * 4) / ms / 1e6, 1)}), flush=True)
        z = np.load(FIX)
        imgs = list(z["rgb"])
        outs = ctx.encode(imgs, make_params(Format.BC1_RGB, Type.UNorm, Quality.Normal))
        sse = [sum(v) for v in zip(*[ctx.decode_sse(o, im, Format.BC1_RGB)[:3] for o, im in zip(outs, imgs)])]
        print(json.dumps({"context": "BC1_RGB Normal", "psnr_crops": round(psnr(sse, sum(im.shape[0] * im.shape[1] for im in imgs), 3), 3)}))


if __name__ == "__main__":
    main()
