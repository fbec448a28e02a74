#!/usr/bin/env python3
"""Ambient occlusion from height maps (csrc/height_ao.hip): its kernel time beside the normal-map
op and the Box mip chain of the same surfaces.

Surfaces resident in HBM: one of 4096^2 and 16 of 2048^2 (--shapes).  The heights are a smooth noise field in red,
rolled per layer, stored as RGBA8, RGBA16F or RGBA32F; the occlusion goes to red of a destination of the same type.
Per case, in one run on the same buffers, as interleaved series (occlusion, normal map, Box chain, occlusion, ...):
  height_ao   cfhip_height_ao_array_device: cfhip_last_kernel_ms -- hipEvents around both launches, summed
  plane       the same call at D = 8, R = 1: the plane pass, the staging and eight direction finishes per texel (a double
              division each) around eight samples -- the floor of the figure above; the plane pass alone is not timed
  normal_map  cfhip_image_ops_device with CFHIP_IMAGE_OP_NORMAL_MAP, one call per layer, kernel times summed
  box_chain   cfhip_generate_mips_array_device, Box, full chain: device events around the call on a stream of the tool's
Best of --steps after a warm-up, and the spread (max - min) of the steps.  samples: texels x the sum of R_d over the
directions; the rate is samples over the kernel time.  The direction and radius grid runs on RGBA8; the other two pixel
types run at D = 16, R = 32.  One JSON line per case, appended to --out.

    python tools/bench_height_ao.py [--steps 5] [--shapes 4096x1,2048x16] [--out profiles/height_ao_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def height_field(n, seed):
    """(n, n) smooth noise in [0, 1]: white noise low-passed in the frequency domain"""
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.standard_normal((n, n)))
    ky, kx = np.meshgrid(np.fft.fftfreq(n), np.fft.rfftfreq(n), indexing="ij")
    f *= np.exp(-(kx*kx + ky*ky)*(n/16.0)**2)
    h = np.fft.irfft2(f, (n, n))
    return ((h - h.min())/(h.max() - h.min())).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", default="4096x1,2048x16")
    ap.add_argument("--directions", default="8,16,32")
    ap.add_argument("--radii", default="8,32,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import height_ao_ref
    from cuttlefish_amd import Context, api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    dirs = [int(v) for v in args.directions.split(",")]
    radii = [int(v) for v in args.radii.split(",")]
    dtypes = {"RGBA8": np.uint8, "RGBA16F": np.float16, "RGBA32F": np.float32}

    def bracket(fn):
        """fn enqueues on `stream`; -> the milliseconds between device events around it"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def series(fns):
        """interleaved: every function once per step, a warm-up step first -> [(best, spread)]"""
        t = [[fn() for fn in fns] for _ in range(args.steps + 1)][1:]
        return [(round(min(c), 4), round(max(c) - min(c), 4)) for c in zip(*t)]

    with Context(0) as ctx:
        for shape in args.shapes.split(","):
            n, layers = (int(v) for v in shape.split("x"))
            field = height_field(n, 1)
            count = int(n).bit_length()
            levels = [[torch.empty((n >> k, n >> k, 4), dtype=torch.float32, device=dev) for k in range(1, count)]
                      for _ in range(layers)]
            lptr = [[t.data_ptr() for t in chain] for chain in levels]
            normal_dst = torch.empty((n, n, 4), dtype=torch.float32, device=dev)
            res = torch.zeros((layers, 4), dtype=torch.int32, device=dev)
            lines = []
            for tname, dtype in dtypes.items():
                img = np.zeros((n, n, 4), np.float32)
                img[..., 0] = field
                img[..., 3] = 1.0
                host = np.round(img*255).astype(np.uint8) if dtype == np.uint8 else img.astype(dtype)
                srcs = [torch.from_numpy(np.roll(host, (37*i, 101*i), (0, 1)).copy()).to(dev) for i in range(layers)]
                dsts = [torch.zeros_like(s) for s in srcs]
                pt, pitch = api.pixel_type_of(host), host.strides[0]
                sp, dp = [t.data_ptr() for t in srcs], [t.data_ptr() for t in dsts]
                ops = api.make_image_ops(ops=api.ImageOp.NormalMap, normal_height=float(n)/64.0)

                def normal_map():
                    total = 0.0
                    for p in sp:
                        ctx.image_ops_device(p, pt, n, n, pitch, ops, normal_dst.data_ptr(), n*16)
                        total += ctx.last_kernel_ms()
                    return total

                def box_chain():
                    return bracket(lambda: ctx.generate_mips_array_device(sp, pt, n, n, pitch, lptr,
                                                                          filter=int(api.ResizeFilter.Box),
                                                                          stream=stream.cuda_stream))

                def occlusion(D, R):
                    def call():
                        ctx.height_ao_device(sp, pt, n, n, pitch, dp, pt, pitch, radius=R, height_scale=float(n)/64.0,
                                             directions=D, results=res.data_ptr())
                        return ctx.last_kernel_ms()
                    return call
                grid = [(D, R) for D in dirs for R in radii] if dtype == np.uint8 else [(16, 32)]
                for D, R in grid:
                    (ao, ao_s), (pl, pl_s), (nm, nm_s), (bx, bx_s) = series([occlusion(D, R), occlusion(8, 1), normal_map,
                                                                              box_chain])
                    vx, vy, _ = height_ao_ref.directions(D)
                    per_texel = sum(height_ao_ref.reach(R, x, y) for x, y in zip(vx, vy))
                    samples = layers*n*n*per_texel
                    rec = res.cpu().numpy().view(api.HEIGHT_AO_RESULT_DTYPE).reshape(-1)
                    row = {"bench": "height_ao", "size": n, "layers": layers, "pixel_type": tname, "directions": D,
                           "radius": R, "steps": args.steps, "launches": 2, "samples_per_texel": per_texel,
                           "occluded": int(rec["occluded"].sum()), "height_ao_kernel_ms": ao, "height_ao_spread_ms": ao_s,
                           "plane_and_d8_r1_scan_ms": pl, "plane_spread_ms": pl_s, "normal_map_kernel_ms": nm,
                           "normal_map_spread_ms": nm_s, "box_chain_ms": bx, "box_chain_spread_ms": bx_s,
                           "height_ao_over_normal_map": round(ao/nm, 2), "height_ao_over_box_chain": round(ao/bx, 2),
                           "samples_per_s": round(samples/(ao*1e-3), 0)}
                    line = json.dumps(row)
                    print(line, flush=True)
                    lines.append(line)
                del srcs, dsts
            if args.out:
                with open(args.out, "a") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
