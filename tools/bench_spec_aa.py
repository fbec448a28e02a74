#!/usr/bin/env python3
"""Specular anti-aliasing (csrc/spec_aa.hip): its time beside the Box mip chain it repairs.

Surfaces resident in HBM: 16 chains of 2048^2.  The normals are RGBA8, the normal map of a smooth noise height field
(tools/spec_aa_quality.py's), rolled per layer; the levels are RGBA32F, 11 of them per chain.  Two cases: `map`, an
RGBA8 roughness map (uniform noise in every channel, green rewritten), and `constant`, no map and a base roughness of
0.3.  In one run, on the same buffers:
  spec_aa    cfhip_spec_aa_array_device: cfhip_last_kernel_ms (hipEvents around every launch, summed), and device
             events around the whole call on a stream of the tool's
  generate   cfhip_generate_mips_array_device of the roughness surfaces (of the normals in `constant`), Box, full chain:
             device events around the call -- the yardstick
Best of --steps after a warm-up, and the spread (max - min) of the steps.  bytes: level 0 read once (4 per texel and
map) plus one float per level texel written; the rate is bytes over the kernel time, beside 8 TB/s.  One JSON line per
case, appended to --out.

    python tools/bench_spec_aa.py [--steps 5] [--size 2048] [--layers 16] [--out profiles/spec_aa_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cuttlefish_amd import Context, api
    from spec_aa_quality import height_field, normals_of
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n, layers = args.size, args.layers

    def bracket(fn):
        """fn enqueues on `stream`; -> the milliseconds between device events around it"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def best(fn):
        t = [fn() for _ in range(args.steps + 1)][1:]
        return round(min(t), 4), round(max(t) - min(t), 4)

    unit = normals_of(height_field(n, 1), 2.0)
    host = np.round(np.concatenate([unit*0.5 + 0.5, np.ones((n, n, 1))], -1)*255).astype(np.uint8)
    rough = np.random.default_rng(2).integers(0, 256, (n, n, 4)).astype(np.uint8)
    normals = [torch.from_numpy(np.roll(host, (37*i, 101*i), (0, 1)).copy()).to(dev) for i in range(layers)]
    maps = [torch.from_numpy(np.roll(rough, (53*i, 11*i), (0, 1)).copy()).to(dev) for i in range(layers)]
    count = int(n).bit_length()
    levels = [[torch.empty((n >> k, n >> k, 4), dtype=torch.float32, device=dev) for k in range(1, count)]
              for _ in range(layers)]
    lptr = [[t.data_ptr() for t in chain] for chain in levels]
    res = torch.zeros((layers*(count - 1), 4), dtype=torch.int32, device=dev)
    level_texels = layers*sum((n >> k)**2 for k in range(1, count))
    lines = []
    with Context(0) as ctx:
        for case in ("map", "constant"):
            kw = dict(channel=1, results=res.data_ptr())
            if case == "map":
                kw.update(rough0=[t.data_ptr() for t in maps], rough_pixel_type=api.PixelType.RGBA8, rough_pitch=n*4)
            else:
                kw.update(base_roughness=0.3)
            src = maps if case == "map" else normals

            def generate():
                return bracket(lambda: ctx.generate_mips_array_device(
                    [t.data_ptr() for t in src], api.PixelType.RGBA8, n, n, n*4, lptr, filter=int(api.ResizeFilter.Box),
                    stream=stream.cuda_stream))

            def kernels():
                ctx.specular_aa_device([t.data_ptr() for t in normals], api.PixelType.RGBA8, n, n, n*4, lptr, **kw)
                return ctx.last_kernel_ms()

            def call():
                return bracket(lambda: ctx.specular_aa_device([t.data_ptr() for t in normals], api.PixelType.RGBA8, n, n,
                                                              n*4, lptr, stream=stream.cuda_stream, **kw))
            gen_ms, gen_spread = best(generate)
            ker_ms, ker_spread = best(kernels)
            call_ms, call_spread = best(call)
            rec = res.cpu().numpy().view(api.SPEC_AA_RESULT_DTYPE).reshape(-1)
            nbytes = layers*n*n*(8 if case == "map" else 4) + 4*level_texels
            row = {"bench": "spec_aa", "case": case, "size": n, "layers": layers, "levels": count - 1,
                   "launches": (count - 1 + 4)//5, "steps": args.steps, "clamped": int(rec["clamped"].sum()),
                   "saturated": int(rec["saturated"].sum()), "spec_aa_kernel_ms": ker_ms,
                   "spec_aa_kernel_spread_ms": ker_spread, "spec_aa_call_ms": call_ms, "spec_aa_call_spread_ms": call_spread,
                   "generate_box_ms": gen_ms, "generate_box_spread_ms": gen_spread,
                   "spec_aa_over_generate": round(ker_ms/gen_ms, 3), "bytes": nbytes,
                   "bytes_per_s": round(nbytes/(ker_ms*1e-3), 0),
                   "fraction_of_8TBps": round(nbytes/(ker_ms*1e-3)/PEAK_BYTES_PER_S, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
