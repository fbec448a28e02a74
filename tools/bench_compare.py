#!/usr/bin/env python3
"""Time of the GPU quality metrics (csrc/compare.hip) against the HBM bound, one JSON line per layout family.

Payloads are the library's own output: a 1024^2 synth.photo tile encoded at Quality.Lowest (BC6H and the UFloat
ASTC row from the tile as float16, the SNorm row from the tile mapped to -1..1), tiled into an 8192^2 block grid.
The reference is the 8192^2 tile as RGBA32F (1 GiB, far above the 256 MiB Infinity Cache).  Each row times
cfhip_compare_device four ways: plain, with the block map, with SSIM, with both.  Timing: cfhip_profile_begin/_end
(hipEvents around each call's launches: Pass A, and with SSIM the decode into scratch, the SSIM pass and the final
reduction).  bytes = payload + reference read (+ block map written); frac_of_8TBps = bytes / time / 8 TB/s.
ssim_flop_per_texel counts the FP64 operations of the SSIM pass's filter and formula per texel, over the compared
channels (a model of the kernel's arithmetic, not a counter reading).

    python tools/bench_compare.py [--steps 8]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth  # noqa: E402

ROWS = [("BC1", 29, 0), ("BC7", 36, 0), ("BC4 s", 33, 1), ("BC5 u", 34, 0), ("EAC RG11", 42, 0),
        ("BC6H UF", 35, 4), ("ASTC 6x6", 47, 0), ("ASTC 6x6 UFloat", 47, 4)]
HBM = 8.0e12
BIG, TILE = 8192, 1024


def tile_payload(payload, fmt, typ, src, dst):
    """the block grid of a src^2 payload tiled to cover dst^2"""
    bw, bh, bb = api.query(fmt, typ)
    sx, sy = (src + bw - 1) // bw, (src + bh - 1) // bh
    dx, dy = (dst + bw - 1) // bw, (dst + bh - 1) // bh
    g = payload.reshape(sy, sx, bb)
    g = np.tile(g, ((dy + sy - 1) // sy, (dx + sx - 1) // sx, 1))[:dy, :dx]
    return np.ascontiguousarray(g).reshape(-1)


def ssim_flops(channels):
    """FP64 operations per texel of the SSIM pass: the horizontal pass (3 products + 5 x 11 multiply-adds on
    26 rows per 16), the vertical pass (5 x 11 multiply-adds) and the formula (about 20)."""
    horiz = (3 + 5 * 11 * 2) * 26.0 / 16.0
    return round(channels * (horiz + 5 * 11 * 2 + 20), 1)


def timed(ctx, fn, steps):
    fn()                                         # warm-up
    torch.cuda.synchronize()
    ctx.profile_begin()
    for _ in range(steps):
        fn()
    ms, n = ctx.profile_end()
    return ms / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tile = synth.photo(TILE, TILE, seed=11)
    tf = tile.astype(np.float32) / 255.0
    ref_np = np.tile(tf, (BIG // TILE, BIG // TILE, 1))
    ref = torch.from_numpy(ref_np).to(dev)
    ref_s = (ref * 2.0 - 1.0).contiguous()
    del ref_np
    res = torch.zeros(ctypes.sizeof(api.CompareResult), dtype=torch.uint8, device=dev)
    with Context(0) as ctx:
        for name, fmt, typ in ROWS:
            src = tf.astype(np.float16) if typ == 4 else (tf * 2.0 - 1.0 if typ == 1 else tile)
            p = ctx.encode([src], make_params(fmt, typ, Quality.Lowest))[0]
            pay = torch.from_numpy(tile_payload(p, fmt, typ, TILE, BIG)).to(dev)
            bw, bh, _ = api.query(fmt, typ)
            nblk = ((BIG + bw - 1) // bw) * ((BIG + bh - 1) // bh)
            emap = torch.empty(nblk, dtype=torch.float32, device=dev)
            r = ref_s if typ == 1 else ref
            layout, _ = api.decoded_layout(fmt, typ)
            torch.cuda.synchronize()

            def run(block_map, ssim):
                ctx.compare_device(pay.data_ptr(), fmt, typ, BIG, BIG, r.data_ptr(), api.PixelType.RGBA32F, BIG * 16,
                                   res.data_ptr(), ssim=ssim, block_errors=emap.data_ptr() if block_map else 0,
                                   block_errors_capacity=nblk if block_map else 0)
            base = pay.numel() + BIG * BIG * 16
            row = {"row": name, "format": Format(fmt).name, "type": Type(typ).name, "layout": layout.name,
                   "size": BIG, "ref": "RGBA32F", "bytes": base}
            for key, bm, ss in (("plain", False, False), ("map", True, False), ("ssim", False, True),
                                ("map_ssim", True, True)):
                ms = timed(ctx, lambda: run(bm, ss), args.steps)
                nbytes = base + (nblk * 4 if bm else 0)
                row[key + "_ms"] = round(ms, 4)
                row[key + "_frac_of_8TBps"] = round(nbytes / (ms * 1e-3) / HBM, 3)
            ch = api.LAYOUT_ARRAY[layout][0]
            row["bound_ms"] = round(base / HBM * 1e3, 4)
            if layout != api.Layout.RGBA16F:
                row["ssim_flop_per_texel"] = ssim_flops(ch)
                row["ssim_extra_ms"] = round(row["ssim_ms"] - row["plain_ms"], 4)
            print(json.dumps(row), flush=True)
            del pay, emap
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
