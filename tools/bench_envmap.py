#!/usr/bin/env python3
"""Environment maps on the GPU (csrc/envmap.hip): the time of each part beside two things the
same cube goes through anyway -- its Box mip chain and its BC6H encode.

Everything is resident in HBM.  The panorama is a smooth sky with noise and one bright sun, RGBA32F.
  equirect   4096 x 2048 -> 512^2 faces, supersample 2: cfhip_last_kernel_ms (hipEvents around the launch)
  prefilter  a 256^2 cube (the panorama at that size), all nine levels, r_k = k / 8, at 256 and at 1024 samples per
             texel: cfhip_last_kernel_ms, summed over the levels; and level 0 alone at roughness 0.5, the 6 x 256^2
             texels of one launch, for the time per fetch
  sh9        64^2 faces: cfhip_last_kernel_ms, both launches
Against, in the same run and on the same cube:
  generate   cfhip_generate_mips_array_device, Box, full chain: device events around the call
  bc6h       cfhip_encode_device of every level of the result, BC6H UFloat, Normal quality: cfhip_last_kernel_ms
Best of --steps after a warm-up, and the spread (max - min) of the steps.  One JSON line per shape, appended to --out.

    python tools/bench_envmap.py [--steps 5] [--out profiles/envmap_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def sky(h, w, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = (0.6 + 0.4*np.sin(x*2.0*np.pi/w + 1.0)*np.cos(y*np.pi/h))[..., None]*np.array([0.9, 1.0, 1.3, 1.0])
    img = img + 0.1*rng.random((h, w, 4))
    img[h//3 - 2:h//3 + 2, (2*w)//3 - 2:(2*w)//3 + 2, :3] = 4.0e3
    return img.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal: every shape 8 times smaller per side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cuttlefish_amd import Context, Format, Quality, Type, api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    shrink = 8 if args.small else 1

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

    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)

    with Context(0) as ctx:
        def cube_of(pano, n):
            faces = torch.empty((6, n, n, 4), dtype=torch.float32, device=dev)

            def run():
                ctx.equirect_to_cube_device(pano.data_ptr(), api.PixelType.RGBA32F, pano.shape[1], pano.shape[0],
                                            pano.shape[1]*16, [faces[f].data_ptr() for f in range(6)], n, 2)
                return ctx.last_kernel_ms()
            return faces, run

        def chain_of(faces):
            n = faces.shape[1]
            L = api.cube_level_count(n)
            chain = [faces] + [torch.empty((6, max(1, n >> l), max(1, n >> l), 4), dtype=torch.float32, device=dev) for l in range(1, L)]

            def run():
                return bracket(lambda: ctx.generate_mips_array_device(
                    [faces[f].data_ptr() for f in range(6)], api.PixelType.RGBA32F, n, n, n*16,
                    [[chain[l][f].data_ptr() for l in range(1, L)] for f in range(6)], filter=int(api.ResizeFilter.Box),
                    stream=stream.cuda_stream))
            return chain, run

        def bc6h_of(levels):
            params = api.make_params(Format.BC6H, Type.UFloat, Quality.Normal)
            surfaces, keep = [], []
            for lvl in levels:
                m = lvl.shape[1]
                for f in range(6):
                    size = api.payload_size(Format.BC6H, Type.UFloat, m, m)
                    out = torch.empty(size, dtype=torch.uint8, device=dev)
                    keep.append(out)
                    surfaces.append(dict(pixels=lvl[f].data_ptr(), pixel_type=api.PixelType.RGBA32F, width=m, height=m,
                                         row_pitch_bytes=m*16, out=out.data_ptr(), out_capacity=size))

            def run():
                ctx.encode_device(surfaces, params)
                return ctx.last_kernel_ms()
            return keep, run

        # ---- panorama to cube
        W, H, n = 4096//shrink, 2048//shrink, 512//shrink
        pano = torch.from_numpy(sky(H, W)).to(dev)
        faces, run = cube_of(pano, n)
        ms, spread = best(run)
        chain, gen = chain_of(faces)
        gen_ms, gen_spread = best(gen)
        keep, enc = bc6h_of(chain)
        enc_ms, enc_spread = best(enc)
        emit({"bench": "envmap", "part": "equirect", "panorama": [W, H], "face": n, "supersample": 2, "steps": args.steps,
              "launches": 1, "fetches": 6*n*n*4*4, "kernel_ms": ms, "kernel_spread_ms": spread,
              "generate_box_ms": gen_ms, "generate_box_spread_ms": gen_spread, "bc6h_kernel_ms": enc_ms,
              "bc6h_kernel_spread_ms": enc_spread, "over_generate": round(ms/gen_ms, 3), "over_bc6h": round(ms/enc_ms, 3)})
        del pano, faces, chain, keep
        torch.cuda.empty_cache()

        # ---- the GGX chain
        W, H, n = 1024//shrink, 512//shrink, 256//shrink
        pano = torch.from_numpy(sky(H, W)).to(dev)
        faces, run = cube_of(pano, n)
        run()
        chain, gen = chain_of(faces)
        gen_ms, gen_spread = best(gen)
        L = len(chain)
        out = [torch.empty_like(c) for c in chain]
        keep, enc = bc6h_of(out)
        src = [[chain[l][f].data_ptr() for l in range(L)] for f in range(6)]
        for samples in (256, 1024):
            roughness = [k/float(L - 1) for k in range(L)]
            tables = [None] + [api.ggx_sample_table(r, samples, n, L) for r in roughness[1:]]

            def whole():
                ctx.cube_prefilter_device(src, n, [[out[k][f].data_ptr() for k in range(L)] for f in range(6)], tables)
                return ctx.last_kernel_ms()
            one = [api.ggx_sample_table(0.5, samples, n, L)]
            top = torch.empty_like(chain[0])

            def level0():
                ctx.cube_prefilter_device(src, n, [[top[f].data_ptr()] for f in range(6)], one)
                return ctx.last_kernel_ms()
            ms, spread = best(whole)
            l0_ms, l0_spread = best(level0)
            enc_ms, enc_spread = best(enc)
            texels = sum(6*max(1, n >> k)**2 for k in range(1, L))
            emit({"bench": "envmap", "part": "prefilter", "face": n, "levels": L, "samples": samples, "steps": args.steps,
                  "launches": L, "filtered_texels": texels, "fetches_at_most": texels*samples*8, "kernel_ms": ms,
                  "kernel_spread_ms": spread, "level0_texels": 6*n*n, "level0_fetches_at_most": 6*n*n*samples*8,
                  "level0_r05_kernel_ms": l0_ms, "level0_r05_kernel_spread_ms": l0_spread,
                  "level0_ns_per_sample": round(l0_ms*1.0e6/(6*n*n*samples), 4),
                  "generate_box_ms": gen_ms, "generate_box_spread_ms": gen_spread, "bc6h_kernel_ms": enc_ms,
                  "bc6h_kernel_spread_ms": enc_spread, "over_generate": round(ms/gen_ms, 3), "over_bc6h": round(ms/enc_ms, 3)})
        del pano, faces, chain, out, keep, top
        torch.cuda.empty_cache()

        # ---- nine coefficients
        W, H, n = 512//shrink, 256//shrink, 64//shrink
        pano = torch.from_numpy(sky(H, W)).to(dev)
        faces, run = cube_of(pano, n)
        run()
        res = torch.zeros(37, dtype=torch.float64, device=dev)

        def sh9():
            ctx.cube_sh9_device([faces[f].data_ptr() for f in range(6)], n, res.data_ptr())
            return ctx.last_kernel_ms()
        ms, spread = best(sh9)
        chain, gen = chain_of(faces)
        gen_ms, gen_spread = best(gen)
        keep, enc = bc6h_of(chain)
        enc_ms, enc_spread = best(enc)
        emit({"bench": "envmap", "part": "sh9", "face": n, "steps": args.steps, "launches": 2, "kernel_ms": ms,
              "kernel_spread_ms": spread, "solid_angle": float(res.cpu().numpy()[36]), "generate_box_ms": gen_ms,
              "generate_box_spread_ms": gen_spread, "bc6h_kernel_ms": enc_ms, "bc6h_kernel_spread_ms": enc_spread,
              "over_generate": round(ms/gen_ms, 3), "over_bc6h": round(ms/enc_ms, 3)})
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
