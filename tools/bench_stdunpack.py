#!/usr/bin/env python3
"""Kernel-only throughput of the standard-format unpack (csrc/std_unpack.hip) next to the packer of the same
(format, type) pair, which moves the same bytes the other way: device-resident buffers, pack and unpack alternating
in the same process, hipEvent timing (cfhip_last_kernel_ms), best and median of N after a warm-up.  Bytes are counted
from the shapes: 16 B of RGBA32F plus the pixel size, per pixel.  One JSON line per (size, pair) with both directions
and their share of the 8 TB/s HBM3E peak; with --compare also the fused compare of R8G8B8A8 UNorm against
cfhip_compare of BC1 at the same size and reference.
usage (GPU box): python tools/bench_stdunpack.py [--sizes 8192,2048] [--steps 20] [--compare] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,2048")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    from cuttlefish_amd import Context, Format, PixelType, Type, api, make_params, payload_size

    ctx = Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def frac(nbytes, ms):
        return round(nbytes/ms/1e6/HBM_PEAK_GBS, 3)

    # one pair of every pixel size: 1, 2, 3, 4, 4 (shared exponent), 6, 8, 12, 16 bytes
    cases = [(Format.R8, Type.UNorm), (Format.R5G6B5, Type.UNorm), (Format.R8G8B8, Type.UNorm),
             (Format.R8G8B8A8, Type.UNorm), (Format.E5B9G9R9_UFloat, Type.UFloat), (Format.R16G16B16, Type.UNorm),
             (Format.R16G16B16A16, Type.Float), (Format.R32G32B32, Type.Float), (Format.R32G32B32A32, Type.Float)]
    for n in [int(v) for v in args.sizes.split(",")]:
        src = torch.rand((n, n, 4), dtype=torch.float32, device="cuda")*1.2 - 0.1
        tex = torch.empty((n, n, 4), dtype=torch.float32, device="cuda")
        for fmt, typ in cases:
            nbytes = payload_size(fmt, typ, n, n)
            pay = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            surf = [{"pixels": src.data_ptr(), "pixel_type": PixelType.RGBA32F, "width": n, "height": n,
                     "row_pitch_bytes": n*16, "out": pay.data_ptr(), "out_capacity": nbytes}]
            p = make_params(fmt, typ, 2)
            pack_ms, unpack_ms = [], []
            for i in range(args.warmup + args.steps):
                ctx.encode_device(surf, p, stream)
                a = ctx.last_kernel_ms()
                ctx.unpack_device(pay.data_ptr(), fmt, typ, n, n, tex.data_ptr(), n*16, stream=stream)
                b = ctx.last_kernel_ms()
                if i >= args.warmup:
                    pack_ms.append(a)
                    unpack_ms.append(b)
            moved = n*n*16 + nbytes
            bp, bu = min(pack_ms), min(unpack_ms)
            emit({"what": "pack_vs_unpack", "format": fmt.name, "type": typ.name, "size": n,
                  "bytes_per_pixel": nbytes//(n*n), "pack_ms": round(bp, 4), "unpack_ms": round(bu, 4),
                  "pack_ms_median": round(statistics.median(pack_ms), 4),
                  "unpack_ms_median": round(statistics.median(unpack_ms), 4),
                  "pack_hbm_frac": frac(moved, bp), "unpack_hbm_frac": frac(moved, bu),
                  "unpack_over_pack": round(bu/bp, 3)})
            del pay
        if args.compare:
            ref = torch.randint(0, 256, (n, n, 4), dtype=torch.uint8, device="cuda")
            res = torch.zeros(ctypes.sizeof(api.CompareResult), dtype=torch.uint8, device="cuda")
            std = torch.randint(0, 256, (n*n*4,), dtype=torch.uint8, device="cuda")
            bc1 = torch.randint(0, 256, (n*n//2,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            std_ms, bc1_ms = [], []
            for i in range(args.warmup + args.steps):
                ctx.compare_std_device(std.data_ptr(), Format.R8G8B8A8, Type.UNorm, n, n, ref.data_ptr(),
                                       PixelType.RGBA8, n*4, res.data_ptr(), stream=stream)
                a = ctx.last_kernel_ms()
                ctx.compare_device(bc1.data_ptr(), Format.BC1_RGB, Type.UNorm, n, n, ref.data_ptr(), PixelType.RGBA8,
                                   n*4, res.data_ptr(), stream=stream)
                b = ctx.last_kernel_ms()
                if i >= args.warmup:
                    std_ms.append(a)
                    bc1_ms.append(b)
            emit({"what": "compare", "size": n, "std_format": "R8G8B8A8", "std_compare_ms": round(min(std_ms), 4),
                  "std_compare_ms_median": round(statistics.median(std_ms), 4),
                  "bc1_compare_ms": round(min(bc1_ms), 4), "bc1_compare_ms_median": round(statistics.median(bc1_ms), 4),
                  "std_hbm_frac": frac(n*n*8, min(std_ms)), "bc1_hbm_frac": frac(n*n*4 + n*n//2, min(bc1_ms))})
        del src, tex
    ctx.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
