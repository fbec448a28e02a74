#!/usr/bin/env python3
"""Kernel time of the GPU decoders (csrc/decode.hip) against the HBM bound, one JSON line per (format, type).

Payloads are the library's own output: a 4096^2 synth.photo tile encoded at Quality.Lowest, tiled 2 x 2 into
an 8192^2 block grid (BC6H from the tile as float16; the SNorm / HDR rows decode the UNorm payload under the
other type -- any bitstream decodes).  Each timed pass decodes one of four distinct 8192^2 surfaces
(payload + texels well above the 256 MiB Infinity Cache), round robin, through cfhip_decode_device; the
SSE rows run cfhip_decode_sse_device against an 8192^2 RGBA8 reference.  Timing: cfhip_profile_begin/_end
(hipEvents around each launch).  bytes = payload read + texels written (decode) or reference read (SSE);
frac_of_8TBps = bytes / kernel time / 8 TB/s.  ms_4096 is the per-launch kernel time on one 4096^2 surface.

    python tools/bench_decode.py [--steps 8] [--formats 36,43]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth  # noqa: E402

PAIRS = ([(f, 0) for f in (29, 30, 31, 32, 36, 37, 38, 39, 40)] + [(f, t) for f in (33, 34, 41, 42) for t in (0, 1)] +
         [(35, 4), (35, 5)] + [(f, t) for f in range(43, 57) for t in (0, 4)])
SSE_LAYOUTS = (api.Layout.RGBA8, api.Layout.R8, api.Layout.RG8)
HBM = 8.0e12
COPIES = 4


def tile_payload(payload, fmt, typ, src, dst):
    """the block grid of a src^2 payload tiled to cover dst^2"""
    bw, bh, bb = api.query(fmt, typ)
    sx, sy = (src + bw - 1) // bw, (src + bh - 1) // bh
    dx, dy = (dst + bw - 1) // bw, (dst + bh - 1) // bh
    g = payload.reshape(sy, sx, bb)
    g = np.tile(g, ((dy + sy - 1) // sy, (dx + sx - 1) // sx, 1))[:dy, :dx]
    return np.ascontiguousarray(g).reshape(-1)


def timed(ctx, fn, steps):
    fn(0)                                        # warm-up
    torch.cuda.synchronize()
    ctx.profile_begin()
    for i in range(steps):
        fn(i)
    ms, n = ctx.profile_end()
    return ms / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--formats", default="")
    args = ap.parse_args()
    only = {int(f) for f in args.formats.split(",") if f}
    dev = torch.device("cuda", 0)
    tile = synth.photo(4096, 4096, seed=11)
    big = 8192
    ref = torch.from_numpy(np.tile(tile, (2, 2, 1))).to(dev)
    sse = torch.zeros(4, dtype=torch.int64, device=dev)
    encoded = {}
    with Context(0) as ctx:
        for fmt, typ in PAIRS:
            if only and fmt not in only:
                continue
            layout, tb = api.decoded_layout(fmt, typ)
            if fmt not in encoded:
                et = Type.UFloat if fmt == Format.BC6H else Type.UNorm
                img = (tile.astype(np.float32) / 255.0).astype(np.float16) if fmt == Format.BC6H else tile
                encoded[fmt] = ctx.encode([img], make_params(fmt, et, Quality.Lowest))[0]
            p4096 = encoded[fmt]
            p8192 = tile_payload(p4096, fmt, 0 if fmt != Format.BC6H else 4, 4096, big)
            d_pay = [torch.from_numpy(p8192).to(dev) for _ in range(COPIES)]
            d_out = [torch.empty(big * big * tb, dtype=torch.uint8, device=dev) for _ in range(COPIES)]
            d_p4 = torch.from_numpy(p4096).to(dev)
            torch.cuda.synchronize()

            def dec(i, n=big, pay=None, out=None):
                k = i % COPIES
                ctx.decode_device((pay if pay is not None else d_pay[k]).data_ptr(), fmt, typ, n, n,
                                  (out if out is not None else d_out[k]).data_ptr(), n * tb)
            ms = timed(ctx, dec, args.steps)
            ms4 = timed(ctx, lambda i: dec(i, 4096, d_p4, d_out[0]), args.steps)
            nbytes = p8192.nbytes + big * big * tb
            row = {"format": Format(fmt).name, "type": Type(typ).name, "layout": layout.name, "size": big,
                   "kernel": ctx.last_kernel_name(), "bytes": nbytes, "kernel_ms": round(ms, 4),
                   "bound_ms": round(nbytes / HBM * 1e3, 4), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / HBM, 3),
                   "ms_4096": round(ms4, 4)}
            if typ == 0 and layout in SSE_LAYOUTS:
                def sse_pass(i, n=big, pay=None):
                    ctx.decode_sse_device((pay if pay is not None else d_pay[i % COPIES]).data_ptr(), fmt, typ, n, n,
                                          ref.data_ptr(), big * 4, sse.data_ptr())
                sms = timed(ctx, sse_pass, args.steps)
                sms4 = timed(ctx, lambda i: sse_pass(i, 4096, d_p4), args.steps)
                sbytes = p8192.nbytes + big * big * 4
                row.update({"sse_bytes": sbytes, "sse_kernel_ms": round(sms, 4),
                            "sse_frac_of_8TBps": round(sbytes / (sms * 1e-3) / HBM, 3), "sse_ms_4096": round(sms4, 4)})
            print(json.dumps(row), flush=True)
            del d_pay, d_out, d_p4
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
