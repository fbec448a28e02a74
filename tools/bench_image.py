#!/usr/bin/env python3
"""Kernel time of the image ops (csrc/image_ops.hip) against the HBM bound, one JSON line per case.

Each timed pass runs cfhip_image_ops_device on one of four distinct 8192^2 surfaces, round robin (source and
destination well above the 256 MiB Infinity Cache).  Timing: cfhip_profile_begin/_end (hipEvents around each
launch).  bytes = source read + RGBA32F destination written; frac_of_8TBps = bytes / kernel time / 8 TB/s.

    python tools/bench_image.py [--steps 8] [--size 8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cuttlefish_amd import Channel, Context, ImageOp as Op, NormalOptions, RotateAngle, api, make_image_ops  # noqa: E402

HBM = 8.0e12
COPIES = 4
SWZ = (Channel.Blue, Channel.Green, Channel.Red, Channel.Alpha)
CASES = [
    ("a_flip_swizzle_premultiply", "f32", dict(ops=Op.FlipX | Op.FlipY | Op.Swizzle | Op.PreMultiply, swizzle=SWZ)),
    ("b_a_plus_rotate90", "f32", dict(ops=Op.FlipX | Op.FlipY | Op.Swizzle | Op.PreMultiply | Op.Rotate, swizzle=SWZ,
                                      rotate=RotateAngle.CW90)),
    ("c_normal_map", "f32", dict(ops=Op.NormalMap, normal_height=2.0)),
    ("c_normal_map_wrap", "f32", dict(ops=Op.NormalMap, normal_height=2.0,
                                      normal_options=NormalOptions.WrapX | NormalOptions.WrapY)),
    ("d_srgb_to_linear_rgba8", "u8", dict(ops=Op.ColorSpace, src_color_space=1, dst_color_space=0)),
    ("d_srgb_to_linear_rgba32f", "f32", dict(ops=Op.ColorSpace, src_color_space=1, dst_color_space=0)),
    ("e_every_op_rgba8", "u8", dict(ops=0xFF, src_color_space=1, dst_color_space=0, rotate=RotateAngle.CCW90,
                                    swizzle=SWZ, normal_height=2.0)),
    ("e_every_op_rgba32f", "f32", dict(ops=0xFF, src_color_space=1, dst_color_space=0, rotate=RotateAngle.CCW90,
                                       swizzle=SWZ, normal_height=2.0)),
]


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
    ap.add_argument("--size", type=int, default=8192)
    args = ap.parse_args()
    n = args.size
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    srcs = {"f32": [torch.rand((n, n, 4), generator=gen, device=dev) for _ in range(COPIES)],
            "u8": [torch.randint(0, 256, (n, n, 4), generator=gen, device=dev, dtype=torch.uint8)
                   for _ in range(COPIES)]}
    dsts = [torch.empty((n, n, 4), dtype=torch.float32, device=dev) for _ in range(COPIES)]
    torch.cuda.synchronize()
    with Context(0) as ctx:
        for name, kind, fields in CASES:
            ops = make_image_ops(**fields)
            pt = api.PixelType.RGBA8 if kind == "u8" else api.PixelType.RGBA32F
            pb = 4 if kind == "u8" else 16

            def run(i):
                k = i % COPIES
                ctx.image_ops_device(srcs[kind][k].data_ptr(), pt, n, n, n * pb, ops, dsts[k].data_ptr(), n * 16)
            ms = timed(ctx, run, args.steps)
            nbytes = n * n * (pb + 16)
            print(json.dumps({"case": name, "size": n, "kernel": ctx.last_kernel_name(), "bytes": nbytes,
                              "kernel_ms": round(ms, 4), "bound_ms": round(nbytes / HBM * 1e3, 4),
                              "frac_of_8TBps": round(nbytes / (ms * 1e-3) / HBM, 3)}), flush=True)


if __name__ == "__main__":
    main()
