#!/usr/bin/env python3
"""The signed distance field from alpha (csrc/alpha_sdf.hip): its time per pass beside alpha
bleeding and a Box mip chain of the same surface, and what it is for -- the edge a small field magnifies to.

Time (the default).  Surfaces resident in HBM: synth.photo seed 1 as a 1024^2 tile repeated, rolled per layer, with
60 opaque discs per 256^2 of surface (about 16 % coverage) over black texels of alpha 0 -- the surface of
tools/bench_alpha_bleed.py.  Three cases: 4096^2 RGBA8, 4096^2 RGBA32F, 2048^2 RGBA8 x 16 layers, each at
(scale, spread) = (1, 8), (8, 16), (16, 64), into an RGBA8 destination.  In one run, on the same buffers:
  sdf       cfhip_alpha_sdf_array_device: cfhip_last_kernel_ms (hipEvents around every launch, summed); and each of
            its launches alone through the library's own launchers, device events around it, on scratch of this tool
  bleed     cfhip_alpha_bleed_array_device, every call from the unbled surface: cfhip_last_kernel_ms
  generate  cfhip_generate_mips_array_device of the same input, Box, full chain: device events around the call
Best of --steps after a warm-up, and the spread (max - min) of the steps.  One JSON line per case and setting, appended
to --out.

Quality (--quality).  Three 256^2 masks (tests/alpha_sdf_ref.py: an off-centre disc, a slanted bar, a five-lobed star)
and the six 128^2 photo crops of tests/golden/pvrtc_photos.npz cut out with the disc of tools/bench_alpha_bleed.py:
the field at scale 8 through the built library, magnified bilinearly by 8 and cut at 0.5, against the mask -- the wrong
texels, beside those of the box-filtered alpha of the same size.  Writes a markdown table to --out.

    python tools/bench_alpha_sdf.py [--steps 5] [--out profiles/alpha_sdf_bench.jsonl]
    python tools/bench_alpha_sdf.py --quality [--out profiles/alpha_sdf_quality.md]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

CASES = (("4096 RGBA8", 4096, 1, np.uint8), ("4096 RGBA32F", 4096, 1, np.float32), ("2048 RGBA8 x 16", 2048, 16, np.uint8))
SETTINGS = ((1, 8), (8, 16), (16, 64))             # (scale, spread)
PASSES = ("classify", "row", "column", "resolve")


class SdfCall(ctypes.Structure):
    """cfsd_call (csrc/alpha_sdf.h)"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_pitch", ctypes.c_ulonglong),
                ("dst_pitch", ctypes.c_ulonglong), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("src_type", ctypes.c_int32), ("dst_type", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("spread", ctypes.c_uint32), ("scale", ctypes.c_uint32), ("channel_mask", ctypes.c_uint32)]


def timing(args):
    import torch
    from bench_alpha_bleed import cutout
    from cuttlefish_amd import Context, api
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lib = api.load_library()
    raw = ctypes.c_void_p(stream.cuda_stream)
    for name in PASSES:
        getattr(lib, "cfhip_launch_alpha_sdf_" + name).restype = ctypes.c_int

    def bracket(fn):
        """fn enqueues on `stream`; -> the milliseconds between device events around it"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def best(fn, steps):
        t = [fn() for _ in range(steps + 1)][1:]
        return round(min(t), 4), round(max(t) - min(t), 4)

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
            texels = layers*n*n
            levels = int(np.log2(n)) + 1
            mips = [[torch.empty((n >> k, n >> k, 4), dtype=torch.float32, device=dev) for k in range(1, levels)]
                    for _ in range(layers)]
            bres = torch.zeros((layers, 4), dtype=torch.int32, device=dev)

            def bleed():
                for w, k in zip(work, keep):
                    w.copy_(k)
                torch.cuda.synchronize(dev)
                ctx.alpha_bleed_device([w.data_ptr() for w in work], pt, n, n, pitch, results=bres.data_ptr())
                return ctx.last_kernel_ms()

            def generate():
                return bracket(lambda: ctx.generate_mips_array_device(
                    [k.data_ptr() for k in keep], pt, n, n, pitch, [[d.data_ptr() for d in c] for c in mips],
                    filter=int(api.ResizeFilter.Box), stream=stream.cuda_stream))
            bleed_ms, bleed_spread = best(bleed, args.steps)
            gen_ms, gen_spread = best(generate, args.steps)
            del work, mips
            for scale, spread in SETTINGS:
                m = n//scale
                dsts = [torch.zeros((m, m, 4), dtype=torch.uint8, device=dev) for _ in range(layers)]
                res = torch.zeros((layers, 4), dtype=torch.int32, device=dev)

                def whole():
                    ctx.alpha_sdf_device([k.data_ptr() for k in keep], pt, n, n, pitch, [d.data_ptr() for d in dsts],
                                         api.PixelType.RGBA8, m*4, spread, scale, results=res.data_ptr())
                    return ctx.last_kernel_ms()
                sdf_ms, sdf_spread = best(whole, args.steps)
                rec = res.cpu().numpy().view(api.SDF_RESULT_DTYPE).reshape(-1)
                # the launches one by one, on scratch of this tool's own
                table = torch.tensor([k.data_ptr() for k in keep] + [d.data_ptr() for d in dsts], dtype=torch.int64, device=dev)
                plane = torch.zeros(layers*n*((n + 63)//64), dtype=torch.int64, device=dev)
                rows = torch.zeros(texels, dtype=torch.uint8, device=dev)
                e = torch.zeros(texels if scale > 1 else 1, dtype=torch.int16, device=dev)
                call = SdfCall(table.data_ptr(), table.data_ptr() + 8*layers, pitch, m*4, n, n, int(pt), int(api.PixelType.RGBA8),
                               0, spread, scale, 8)
                ref, p = ctypes.byref(call), ctypes.c_void_p
                launch = {
                    "classify": lambda: lib.cfhip_launch_alpha_sdf_classify(ref, layers, ctypes.c_float(0.5), p(plane.data_ptr()),
                                                                            p(res.data_ptr()), raw),
                    "row": lambda: lib.cfhip_launch_alpha_sdf_row(ref, layers, p(plane.data_ptr()), p(rows.data_ptr()), raw),
                    "column": lambda: lib.cfhip_launch_alpha_sdf_column(ref, layers, p(rows.data_ptr()), p(e.data_ptr()),
                                                                        p(res.data_ptr()), raw),
                    "resolve": lambda: lib.cfhip_launch_alpha_sdf_resolve(ref, layers, p(e.data_ptr()), raw)}
                passes = {}
                for which in PASSES[:4 if scale > 1 else 3]:
                    def one(which=which):
                        return bracket(lambda: launch[which]() == 0 or sys.exit("launch of %s failed" % which))
                    passes[which] = best(one, args.steps)
                torch.cuda.synchronize(dev)
                row = {"bench": "alpha_sdf", "case": name, "size": n, "layers": layers, "source": np.dtype(dtype).name,
                       "coverage": round(cover, 4), "steps": args.steps, "scale": scale, "spread": spread,
                       "launches": 3 if scale == 1 else 4, "inside": int(rec["inside"].sum()),
                       "saturated": int(rec["saturated"].sum()),
                       "scratch_bytes": layers*n*((n + 63)//64)*8 + texels*(3 if scale > 1 else 1),
                       "sdf_kernel_ms": sdf_ms, "sdf_kernel_spread_ms": sdf_spread}
                for which, (ms, sp) in passes.items():
                    row[which + "_ms"] = ms
                    row[which + "_spread_ms"] = sp
                row.update({"bleed_kernel_ms": bleed_ms, "bleed_kernel_spread_ms": bleed_spread,
                            "generate_box_ms": gen_ms, "generate_box_spread_ms": gen_spread,
                            "sdf_over_bleed": round(sdf_ms/bleed_ms, 3), "sdf_over_generate": round(sdf_ms/gen_ms, 3)})
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                del dsts, table, plane, rows, e
            del keep
            torch.cuda.empty_cache()
            if args.size:
                break
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def quality(args):
    import alpha_sdf_ref as R
    from cuttlefish_amd import Context
    masks = dict(R.shapes())
    crops = np.load(os.path.join(ROOT, "tests", "golden", "pvrtc_photos.npz"))["rgb"]
    y, x = np.mgrid[0:128, 0:128]
    disc = (x - 64)**2 + (y - 60)**2 <= 44**2
    images = {}
    for name, mask in masks.items():
        img = np.zeros(mask.shape + (4,), np.uint8)
        img[..., 3] = mask*255
        images[name] = (img, mask)
    for i, crop in enumerate(crops):
        img = crop.copy()
        img[~disc] = 0
        img[disc, 3] = 255
        images["photo crop %d under a disc" % i] = (img, disc)
    out = ["# The distance field: the edge a small texture magnifies to",
           "",
           "`tools/bench_alpha_sdf.py --quality`, on the GPU.  A mask is reduced to 1/8 per side, magnified bilinearly by 8",
           "(texel centres, clamped) and cut at 0.5; the figure is the number of texels that differ from the mask.  `field`:",
           "`Context.alpha_sdf` at scale 8, RGBA8 output, at spread 8 and 16.  `box alpha`: the mask's 8-bit alpha",
           "box-filtered to the same size.  The 256x256 masks are those of `tests/alpha_sdf_ref.py`; the 128x128 photo crops of",
           "`tests/golden/pvrtc_photos.npz` are cut out with a disc of radius 44 (alpha 255 inside, 0 outside).",
           "",
           "| mask | size | field, spread 8 | field, spread 16 | box alpha |",
           "|---|---|---|---|---|"]
    with Context(0) as ctx:
        for name, (img, mask) in images.items():
            wrong = []
            for spread in (8, 16):
                field, _ = ctx.alpha_sdf(img, spread, 8)
                wrong.append(R.mismatches(field[..., 3]/255.0, mask))
            out.append("| %s | %dx%d | %d | %d | %d |" % (name, mask.shape[1], mask.shape[0], wrong[0], wrong[1],
                                                       R.mismatches(R.box_alpha(mask, 8), mask)))
    text = "\n".join(out) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=0, help="time one case only: RGBA8 at this size (a rehearsal)")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (quality if args.quality else timing)(args)


if __name__ == "__main__":
    main()
