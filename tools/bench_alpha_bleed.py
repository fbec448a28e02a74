#!/usr/bin/env python3
"""Alpha bleeding (csrc/alpha_bleed.hip): its time beside the mip chain it sits in front of, and
what it does to the chain and to the block encoders.

Time (the default).  Surfaces resident in HBM: synth.photo seed 1 as a 1024^2 tile repeated, rolled per layer, with
60 opaque discs per 256^2 of surface (about 16 % coverage) over black texels of alpha 0.  Three cases: 4096^2 RGBA32F,
4096^2 RGBA8, 2048^2 RGBA8 x 16 layers.  In one run, on the same buffers:
  bleed      cfhip_alpha_bleed_array_device: cfhip_last_kernel_ms (hipEvents around every launch, summed) and device
             events around the whole call on the stream; every timed call starts from the unbled surface
  generate  cfhip_generate_mips_array_device of the same input, CatmullRom, full chain: device events around the call
--steps runs after a warm-up; the minimum and the spread (max - min).  bytes_min: what the passes must move at the
least -- per texel 4 B written by the seed pass, 4 B read + 4 B written by each step, 4 B read by the fill, plus the
alpha read (a whole texel's cache line share) and the colours copied -- and the time that takes at 8 TB/s.
One JSON line per case, appended to --out.

Quality (--quality).  The six 128^2 photo crops of tests/golden/pvrtc_photos.npz cut out with a disc (alpha 255 inside,
colour and alpha 0 outside), with and without Texture.bleed_alpha(): PSNR of the visible texels (level alpha > 0.25) of
every generated level against the alpha-weighted colour of the level-0 texels under them, for Box and CatmullRom, and
PSNR over the texels with alpha > 0 of level 0 after BC3 and BC7 at Quality.Normal.  Writes a markdown table to --out.

    python tools/bench_alpha_bleed.py [--steps 5] [--out profiles/alpha_bleed_bench.jsonl]
    python tools/bench_alpha_bleed.py --quality [--out profiles/alpha_bleed_quality.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CASES = (("4096 RGBA32F", 4096, 1, np.float32), ("4096 RGBA8", 4096, 1, np.uint8), ("2048 RGBA8 x 16", 2048, 16, np.uint8))


def cutout(n, seed=5):
    """(n, n, 4) uint8: the photo tile under 60 discs per 256^2, black and transparent elsewhere"""
    from cuttlefish_amd import synth
    tile = synth.photo(1024, 1024, seed=1)
    base = np.tile(tile, (max(1, n//1024), max(1, n//1024), 1))[:n, :n].copy()
    rng = np.random.default_rng(seed)
    mask = np.zeros((n, n), bool)
    y, x = np.mgrid[0:256, 0:256]
    for ty in range(0, n, 256):                    # disc centres per 256^2 cell; a disc stays inside its cell's array
        for tx in range(0, n, 256):
            cell = np.zeros((256, 256), bool)
            for _ in range(60):
                cy, cx, r = rng.integers(256), rng.integers(256), rng.integers(3, 13)
                cell |= (x - cx)**2 + (y - cy)**2 <= r*r
            mask[ty:ty + 256, tx:tx + 256] = cell[:n - ty, :n - tx]
    base[~mask] = 0
    base[mask, 3] = 255
    return base, float(mask.mean())


def timing(args):
    import torch
    from cuttlefish_amd import Context, api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def bracket(fn):
        """fn enqueues on `stream`; -> the milliseconds between device events around it"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    lines = []
    with Context(0) as ctx:
        for name, n, layers, dtype in CASES:
            if args.size:
                n = args.size
            base, cover = cutout(n)
            host = base if dtype == np.uint8 else (base.astype(np.float32)/np.float32(255))
            keep = [torch.from_numpy(np.roll(host, (37*i, 101*i), (0, 1)).copy()).to(dev) for i in range(layers)]
            work = [k.clone() for k in keep]
            pt = api.pixel_type_of(host)
            pitch = host.strides[0]
            res = torch.zeros((layers, 4), dtype=torch.int32, device=dev)
            levels = int(np.log2(n)) + 1
            dsts = [[torch.empty((n >> k, n >> k, 4), dtype=torch.float32, device=dev) for k in range(1, levels)]
                    for _ in range(layers)]

            def bleed():
                ctx.alpha_bleed_device([w.data_ptr() for w in work], pt, n, n, pitch, results=res.data_ptr(),
                                       stream=stream.cuda_stream)

            def generate():
                ctx.generate_mips_array_device([w.data_ptr() for w in work], pt, n, n, pitch,
                                               [[d.data_ptr() for d in c] for c in dsts],
                                               filter=int(api.ResizeFilter.CatmullRom), stream=stream.cuda_stream)
            kernel, wall = [], []
            for _ in range(args.steps + 1):
                for w, k in zip(work, keep):
                    w.copy_(k)
                torch.cuda.synchronize(dev)
                wall.append(bracket(bleed))
                kernel.append(ctx.last_kernel_ms())
            kernel, wall = kernel[1:], wall[1:]
            rec = res.cpu().numpy().view(api.BLEED_RESULT_DTYPE).reshape(-1)
            gen = [bracket(generate) for _ in range(args.steps + 1)][1:]
            texels = layers*n*n
            passes = int(np.log2(n)) + 2
            texel = host.itemsize*4
            filled = int(rec["filled"].sum())
            # seed: alpha read (its share of the cache line: the whole texel) + 4 B; steps: 8 B; fill: 4 B + rgb read + rgb written
            bytes_min = texels*(texel + 4) + (passes - 2)*texels*8 + texels*4 + filled*2*(texel*3//4)
            row = {"bench": "alpha_bleed", "case": name, "size": n, "layers": layers, "source": np.dtype(dtype).name,
                   "coverage": round(cover, 4), "steps": args.steps, "launches": passes,
                   "seeds": int(rec["seeds"].sum()), "filled": filled, "max_dist2": int(rec["max_dist2"].max()),
                   "scratch_bytes": texels*8,
                   "bleed_kernel_ms": round(min(kernel), 4), "bleed_kernel_spread_ms": round(max(kernel) - min(kernel), 4),
                   "bleed_stream_ms": round(min(wall), 4), "bleed_stream_spread_ms": round(max(wall) - min(wall), 4),
                   "generate_catmullrom_ms": round(min(gen), 4), "generate_spread_ms": round(max(gen) - min(gen), 4),
                   "bleed_over_generate": round(min(wall)/min(gen), 3),
                   "bytes_min": bytes_min, "ms_at_8TBps": round(bytes_min/8e12*1e3, 4),
                   "achieved_TBps_of_bytes_min": round(bytes_min/(min(kernel)*1e-3)/1e12, 3)}
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del keep, work, dsts
            torch.cuda.empty_cache()
            if args.size:
                break
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def psnr(err2_sum, count):
    return float("inf") if err2_sum == 0 else 10.0*np.log10(count/err2_sum)


def quality(args):
    from cuttlefish_amd import Format, Quality, ResizeFilter, Texture, Type
    crops = np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]
    y, x = np.mgrid[0:128, 0:128]
    disc = (x - 64)**2 + (y - 60)**2 <= 44**2
    levels = range(1, 6)
    # [filter][bled][level] -> (squared error, values); [format][bled] -> the same
    chain = {f: {b: {k: [0.0, 0] for k in levels} for b in (False, True)} for f in ("Box", "CatmullRom")}
    enc = {f: {b: [0.0, 0] for b in (False, True)} for f in ("BC3", "BC7")}
    for crop in crops:
        img = crop.copy()
        img[~disc] = 0
        img[disc, 3] = 255
        b64 = img.astype(np.float64)/255.0
        for bled in (False, True):
            for fname in chain:
                t = Texture(128, 128)
                assert t.set_image(img.copy())
                assert not bled or t.bleed_alpha()
                assert t.generate_mipmaps(getattr(ResizeFilter, fname))
                for k in levels:
                    n = 128 >> k
                    blocks = b64.reshape(n, 1 << k, n, 1 << k, 4)
                    wsum = blocks[..., 3].sum((1, 3))
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ref = (blocks[..., :3]*blocks[..., 3:]).sum((1, 3))/wsum[..., None]
                    lvl = t.get_image(k).astype(np.float64)
                    vis = (lvl[..., 3] > 0.25) & (wsum > 0)
                    e = chain[fname][bled][k]
                    e[0] += float(((lvl[..., :3] - ref)[vis]**2).sum())
                    e[1] += int(vis.sum())*3
            for fname in enc:
                t = Texture(128, 128)
                assert t.set_image(img.copy())
                assert not bled or t.bleed_alpha()
                assert t.convert(getattr(Format, fname), Type.UNorm, Quality.Normal)
                dec = t.decode_image(0).astype(np.float64)
                e = enc[fname][bled]
                e[0] += float(((dec[..., :3] - b64[..., :3])[disc]**2).sum())
                e[1] += int(disc.sum())*3
    out = ["# Alpha bleeding: what it does to the mip chain and to the block encoders",
           "",
           "`tools/bench_alpha_bleed.py --quality`, on the GPU.  Input: the six 128x128 photo crops of",
           "`tests/golden/pvrtc_photos.npz`, each cut out with a disc of radius 44 (alpha 255 inside; colour and alpha 0",
           "outside, as an exporter leaves them), with and without `Texture.bleed_alpha()` in front.  All six crops pooled.",
           "",
           "## Generated levels",
           "",
           "PSNR (peak 1.0) of the R, G, B of the visible texels of each level (level alpha > 0.25) against the",
           "alpha-weighted colour of the level-0 texels under them, `sum(alpha * c) / sum(alpha)` over the 2^k x 2^k block.",
           "For CatmullRom that reference is not the filter's own footprint, so the figure has a floor that bleeding",
           "cannot lift: the difference between the two filters on the opaque interior.",
           "",
           "| filter | level | size | plain dB | bled dB |",
           "|---|---|---|---|---|"]
    for fname in chain:
        for k in levels:
            p, b = chain[fname][False][k], chain[fname][True][k]
            out.append("| %s | %d | %dx%d | %.2f | %.2f |" % (fname, k, 128 >> k, 128 >> k, psnr(*p), psnr(*b)))
    out += ["",
            "## Block encoders, level 0, Quality.Normal",
            "",
            "PSNR (peak 1.0) of the decoded R, G, B against the source over the texels with alpha > 0: the blocks on the",
            "silhouette no longer fit their endpoints to black texels nobody sees.",
            "",
            "| format | plain dB | bled dB |",
            "|---|---|---|"]
    for fname in enc:
        out.append("| %s | %.2f | %.2f |" % (fname, psnr(*enc[fname][False]), psnr(*enc[fname][True])))
    text = "\n".join(out) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=0, help="time one case only: RGBA32F at this size (a rehearsal)")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (quality if args.quality else timing)(args)


if __name__ == "__main__":
    main()
