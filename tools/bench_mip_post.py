#!/usr/bin/env python3
"""The mip post-pass (csrc/mip_post.hip) beside the generation of the chains it repairs.

16 chains of 2048^2 RGBA8 with full chains (12 levels), resident in HBM: synth.photo seed 1 as a 1024^2 tile repeated,
rolled per chain, alpha a cut-out mask (255 where green is above its median).  In one run, on the same buffers:
  generate   cfhip_generate_mips_array_device, Box: device events around the call's launches on one stream (the entry
             has no per-launch events of its own)
  coverage / normals / both
             cfhip_mip_post_array_device at threshold 0.5: cfhip_last_kernel_ms (hipEvents around every launch, summed)
             and, for the same footing as `generate`, device events around the whole call on the stream
Every timed post-pass starts from the levels as generated (restored from a copy outside the timed window: a second pass
over repaired levels would find nothing to do).  --steps runs after a warm-up; the minimum and the spread (max - min).
One JSON line, appended to --out.

    python tools/bench_mip_post.py [--steps 5] [--out profiles/mip_post_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cuttlefish_amd import Context, api, synth
    dev = torch.device("cuda", 0)
    n, chains = args.size, args.chains
    tile = synth.photo(1024, 1024, seed=1)
    base = np.tile(tile, (max(1, n//1024), max(1, n//1024), 1))[:n, :n].copy()
    base[..., 3] = np.where(base[..., 1] > np.median(base[..., 1]), 255, 0)
    levels = int(np.log2(n)) + 1
    srcs = [torch.from_numpy(np.roll(base, (37*i, 101*i), (0, 1)).copy()).to(dev) for i in range(chains)]
    dsts = [[torch.empty((n >> k, n >> k, 4), dtype=torch.float32, device=dev) for k in range(1, levels)] for _ in range(chains)]
    res = torch.zeros((chains*(levels - 1), 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    texels = chains*sum((n >> k)**2 for k in range(1, levels))

    def bracket(fn):
        """fn enqueues on `stream`; -> the milliseconds between device events around it"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    with Context(0) as ctx:
        def generate():
            ctx.generate_mips_array_device([s.data_ptr() for s in srcs], api.PixelType.RGBA8, n, n, n*4,
                                           [[d.data_ptr() for d in c] for c in dsts], filter=0, stream=stream.cuda_stream)
        gen = [bracket(generate) for _ in range(args.steps + 1)][1:]
        keep = [[d.clone() for d in c] for c in dsts]
        row = {"bench": "mip_post", "size": n, "chains": chains, "levels": levels, "source": "uint8", "threshold": 0.5,
               "level_texels": texels, "steps": args.steps,
               "generate_ms": round(min(gen), 4), "generate_spread_ms": round(max(gen) - min(gen), 4)}
        for name, kw in (("coverage", dict(alpha_coverage=0.5)), ("normals", dict(normalize="unorm")),
                         ("both", dict(alpha_coverage=0.5, normalize="unorm"))):
            def post():
                ctx.mip_post_device([s.data_ptr() for s in srcs], api.PixelType.RGBA8, n, n, n*4,
                                    [[d.data_ptr() for d in c] for c in dsts], results=res.data_ptr(),
                                    stream=stream.cuda_stream, **kw)
            kernel, wall = [], []
            for _ in range(args.steps + 1):
                for c, k in zip(dsts, keep):
                    for d, s in zip(c, k):
                        d.copy_(s)
                torch.cuda.synchronize(dev)
                wall.append(bracket(post))
                kernel.append(ctx.last_kernel_ms())
            kernel, wall = kernel[1:], wall[1:]
            row[name + "_kernel_ms"] = round(min(kernel), 4)
            row[name + "_kernel_spread_ms"] = round(max(kernel) - min(kernel), 4)
            row[name + "_stream_ms"] = round(min(wall), 4)
            row[name + "_over_generate"] = round(min(wall)/min(gen), 3)
            if "alpha_coverage" in kw:
                rec = res.cpu().numpy().view(api.MIP_POST_RESULT_DTYPE).reshape(chains, levels - 1)
                row[name + "_levels_scaled"] = int((rec["scale"] != 1).sum())
                row[name + "_chain0_scales"] = [round(float(s), 4) for s in rec["scale"][0]]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
