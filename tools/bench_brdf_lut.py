#!/usr/bin/env python3
"""The BRDF lookup table, the irradiance cube and a Charlie chain on the GPU (csrc/envmap.hip),
each beside the GGX chain of the same 256^2 cube for scale (section 4.23's figure, measured again in the same run).

Everything is resident in HBM; every figure is cfhip_last_kernel_ms (hipEvents around the launches).
  lut         128^2 and 256^2 texels, 1024 samples, with and without the sheen column: one launch, a wavefront per texel
  irradiance  32^2 faces from the nine coefficients of a 64^2 cube: one launch
  chains      a 256^2 cube (a smooth sky with one sun), all nine levels, level 0 a copy, 1024 samples: the GGX chain at
              r_k = k / 8 and a Charlie chain at r_k from 0.3 to 1 (a sharper sheen level leaves none of 1024 records
              above the horizon) -- the same kernel, another table
Best of --steps after a warm-up, and the spread (max - min) of the steps.  One JSON line per shape, appended to --out.

    python tools/bench_brdf_lut.py [--steps 5] [--out profiles/brdf_lut_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a rehearsal: every shape 8 times smaller per side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_envmap import sky
    from cuttlefish_amd import Context, api
    dev = torch.device("cuda", 0)
    shrink = 8 if args.small else 1

    def best(fn):
        t = [fn() for _ in range(args.steps + 1)][1:]
        return round(min(t), 4), round(max(t) - min(t), 4)

    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)

    with Context(0) as ctx:
        # ---- the GGX chain and the Charlie chain of one cube
        W, H, n, samples = 1024//shrink, 512//shrink, 256//shrink, 1024
        pano = torch.from_numpy(sky(H, W)).to(dev)
        faces = torch.empty((6, n, n, 4), dtype=torch.float32, device=dev)
        ctx.equirect_to_cube_device(pano.data_ptr(), api.PixelType.RGBA32F, W, H, W*16, [faces[f].data_ptr() for f in range(6)], n, 2)
        L = api.cube_level_count(n)
        chain = [faces] + [torch.empty((6, max(1, n >> l), max(1, n >> l), 4), dtype=torch.float32, device=dev) for l in range(1, L)]
        ctx.generate_mips_array_device([faces[f].data_ptr() for f in range(6)], api.PixelType.RGBA32F, n, n, n*16,
                                       [[chain[l][f].data_ptr() for l in range(1, L)] for f in range(6)],
                                       filter=int(api.ResizeFilter.Box))
        out = [torch.empty_like(c) for c in chain]
        src = [[chain[l][f].data_ptr() for l in range(L)] for f in range(6)]
        dst = [[out[k][f].data_ptr() for k in range(L)] for f in range(6)]
        ramps = {"ggx": [k/float(L - 1) for k in range(1, L)],
                 "charlie": [0.3 + 0.7*(k - 1)/float(max(L - 2, 1)) for k in range(1, L)]}
        chain_ms = {}
        for name, kind in (("ggx", api.LOBE_GGX), ("charlie", api.LOBE_CHARLIE)):
            tables = [None] + [api.lobe_sample_table(kind, r, samples, n, L) for r in ramps[name]]

            def whole():
                ctx.cube_prefilter_device(src, n, dst, tables)
                return ctx.last_kernel_ms()
            chain_ms[name] = best(whole)
            weighted = [int((t[:, 2] > 0).sum()) for t in tables[1:]]
            emit({"bench": "brdf_lut", "part": "chain", "lobe": name, "face": n, "levels": L, "samples": samples,
                  "roughness": [round(r, 4) for r in ramps[name]], "steps": args.steps, "launches": L,
                  "weighted_records": weighted, "kernel_ms": chain_ms[name][0], "kernel_spread_ms": chain_ms[name][1], "finite": bool(all(torch.isfinite(o).all().item() for o in out))})
        ggx_ms = chain_ms["ggx"][0]
        del pano, chain, out
        torch.cuda.empty_cache()

        # ---- the lookup table
        table = api.hammersley_table(samples)
        for size in (128//shrink, 256//shrink):
            lut = torch.empty((size, size, 4), dtype=torch.float32, device=dev)
            for sheen in (False, True):
                def run():
                    ctx.brdf_lut_device(lut.data_ptr(), size, size, table, sheen)
                    return ctx.last_kernel_ms()
                ms, spread = best(run)
                emit({"bench": "brdf_lut", "part": "lut", "size": size, "samples": samples, "sheen": sheen, "steps": args.steps,
                      "launches": 1, "kernel_ms": ms, "kernel_spread_ms": spread,
                      "ns_per_sample": round(ms*1.0e6/(size*size*samples), 5),
                      "ggx_chain_256_ms": ggx_ms, "over_ggx_chain": round(ms/ggx_ms, 3)})

        # ---- the irradiance cube
        n0, m = 64//shrink, 32//shrink
        res = torch.zeros(37, dtype=torch.float64, device=dev)
        small = faces[:, :n0, :n0].contiguous()
        ctx.cube_sh9_device([small[f].data_ptr() for f in range(6)], n0, res.data_ptr())
        cube = torch.empty((6, m, m, 4), dtype=torch.float32, device=dev)

        def irradiance():
            ctx.cube_irradiance_device(res.data_ptr(), [cube[f].data_ptr() for f in range(6)], m, True)
            return ctx.last_kernel_ms()
        ms, spread = best(irradiance)
        emit({"bench": "brdf_lut", "part": "irradiance", "face": m, "steps": args.steps, "launches": 1, "kernel_ms": ms,
              "kernel_spread_ms": spread, "ggx_chain_256_ms": ggx_ms, "over_ggx_chain": round(ms/ggx_ms, 5)})
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
