#!/usr/bin/env python3
"""Time of the GPU quality metrics (csrc/compare.hip) against the HBM bound, one JSON line per layout family.

Payloads are the library's own output: a 1024^2 synth.photo tile encoded at Quality.Lowest (BC6H and the UFloat
ASTC row from the tile as float16, the SNorm row from the tile mapped to -1..1), tiled into an 8192^2 block grid.
The reference is the 8192^2 tile as RGBA32F (1 GiB, far above the 256 MiB Infinity Cache).  Each row times
cfhip_compare_device four ways: plain, with the block map, with SSIM, with both.  Timing: cfhip_profile_begin/_end
(hipEvents around each call's launches: Pass A, and with SSIM the decode into scratch, the SSIM pass and the final
reduction).  bytes = payload + reference read (+ block map written); frac_of_8TBps = bytes / time / 8 TB/s.
ssim_flop_per_texel counts the FP64 operations of the SSIM pass's filter and formula per texel, over the compared
channels (a model of the kernel's arithmetic, not a counter reading).

    python tools/bench_compare.py [--steps 8]

--batch measures the batched compare instead, the per-surface route and the batched route
alternating in one process, each figure the best of --steps runs after a warm-up, with spread = max - min:
  * one 8192^2 surface, RGBA32F reference, device buffers: cfhip_compare_device against a cfhip_compare_batch_device
    of one surface (kernel ms, with SSIM and without);
  * whole textures from host memory, RGBA8 references: a loop of Context.compare against one Context.compare_batch
    (summed kernel ms and wall ms, with SSIM and without);
  * Texture.convert() + compare() against convert_and_compare(), and Texture.transcode() + a compare through the
    host against transcode(measure=True) (wall ms, SSIM on); the two-call routes are timed twice, with the compare
    one Context.compare per surface (Texture.compare before the batched entry existed) and with Texture.compare
    as it is now.

    python tools/bench_compare.py --batch [--steps 10] [--only single,chains,convert,transcode]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import Context, CubeFace, Dimension, Format, Quality, Texture, Type, api, make_params, synth  # noqa: E402

ROWS = [("BC1", 29, 0), ("BC7", 36, 0), ("BC4 s", 33, 1), ("BC5 u", 34, 0), ("EAC RG11", 42, 0),
        ("BC6H UF", 35, 4), ("ASTC 6x6", 47, 0), ("ASTC 6x6 UFloat", 47, 4)]
HBM = 8.0e12
BIG, TILE = 8192, 1024


def tile_payload(payload, fmt, typ, src, dst):
    """the block grid of a src^2 payload tiled to cover dst^2"""
    bw, bh, bb = api.query(fmt, typ)
    sx, sy = (src + bw - 1) // bw, (src + bh - 1) // bh
    dx, dy = (dst + bw - 1) // bw, (dst + bh - 1) // bh
    g = payload.reshape(sy, sx, bb)
    g = np.tile(g, ((dy + sy - 1) // sy, (dx + sx - 1) // sx, 1))[:dy, :dx]
    return np.ascontiguousarray(g).reshape(-1)


def ssim_flops(channels):
    """FP64 operations per texel of the SSIM pass: the horizontal pass (3 products + 5 x 11 multiply-adds on
    26 rows per 16), the vertical pass (5 x 11 multiply-adds) and the formula (about 20)."""
    horiz = (3 + 5 * 11 * 2) * 26.0 / 16.0
    return round(channels * (horiz + 5 * 11 * 2 + 20), 1)


def timed(ctx, fn, steps):
    fn()                                         # warm-up
    torch.cuda.synchronize()
    ctx.profile_begin()
    for _ in range(steps):
        fn()
    ms, n = ctx.profile_end()
    return ms / max(n, 1)


def alternate(routes, steps):
    """{name: [figures of each run]} of the routes run in turn, steps times after one warm-up round; a route
    returns one figure or a dict of them"""
    for fn in routes.values():
        fn()
    runs = {k: [] for k in routes}
    for _ in range(steps):
        for k, fn in routes.items():
            runs[k].append(fn())
    out = {}
    for k, vals in runs.items():
        keys = vals[0].keys() if isinstance(vals[0], dict) else [None]
        for sub in keys:
            v = [x[sub] for x in vals] if sub is not None else vals
            name = k if sub is None else "%s_%s" % (k, sub)
            out[name + "_best"] = round(min(v), 4)
            out[name + "_spread"] = round(max(v) - min(v), 4)
    return out


def level_images(tile, size, levels):
    """`levels` RGBA8 images size, size/2, ...: the tile repeated (or cut) to each size"""
    out = []
    for m in range(levels):
        s = max(1, size >> m)
        reps = (s + tile.shape[0] - 1) // tile.shape[0]
        out.append(np.ascontiguousarray(np.tile(tile, (reps, reps, 1))[:s, :s]))
    return out


def batch_single(ctx, steps, tile, dev):
    tf = tile.astype(np.float32) / 255.0
    ref = torch.from_numpy(np.tile(tf, (BIG // TILE, BIG // TILE, 1))).to(dev)
    size = ctypes.sizeof(api.CompareResult)
    res = torch.zeros(size, dtype=torch.uint8, device=dev)
    for name, fmt in (("BC7", 36), ("ASTC 6x6", 47)):
        p = ctx.encode([tile], make_params(fmt, 0, Quality.Lowest))[0]
        pay = torch.from_numpy(tile_payload(p, fmt, 0, TILE, BIG)).to(dev)
        torch.cuda.synchronize()
        for ssim in (False, True):
            def single():
                ctx.compare_device(pay.data_ptr(), fmt, 0, BIG, BIG, ref.data_ptr(), api.PixelType.RGBA32F, BIG * 16,
                                   res.data_ptr(), ssim=ssim)
                return ctx.last_kernel_ms()

            def batch():
                ctx.compare_batch_device([dict(blocks=pay.data_ptr(), ref=ref.data_ptr(), width=BIG, height=BIG,
                                               ref_pitch_bytes=BIG * 16)], fmt, 0, api.PixelType.RGBA32F,
                                         res.data_ptr(), ssim=ssim)
                return ctx.last_kernel_ms()
            row = {"row": "single", "format": name, "size": BIG, "ref": "RGBA32F", "ssim": ssim, "unit": "kernel ms"}
            row.update(alternate({"per_surface": single, "batch_of_one": batch}, steps))
            print(json.dumps(row), flush=True)
        del pay
    del ref
    torch.cuda.empty_cache()


def batch_chains(ctx, steps, tile):
    cases = [("BC7 4096^2 chain", 36, [level_images(tile, 4096, 13)]),
             ("BC3 1024^2 cube chain", 32, [level_images(tile, 1024, 11) for _ in range(6)]),
             ("16 x ASTC 6x6 2048^2 chains", 47, [level_images(tile, 2048, 12) for _ in range(16)])]
    for name, fmt, chains in cases:
        refs = [im for chain in chains for im in chain]
        pays = ctx.encode(refs, make_params(fmt, 0, Quality.Lowest))
        for ssim in (False, True):
            def loop():
                t0, ms = time.perf_counter(), 0.0
                for p, r in zip(pays, refs):
                    ctx.compare(p, r, fmt, 0, ssim=ssim)
                    ms += ctx.last_kernel_ms()
                return {"kernel_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3}

            def batch():
                t0 = time.perf_counter()
                ctx.compare_batch(pays, refs, fmt, 0, ssim=ssim)
                wall = (time.perf_counter() - t0) * 1e3
                return {"kernel_ms": ctx.last_kernel_ms(), "wall_ms": wall}
            row = {"row": "chains", "texture": name, "surfaces": len(refs), "ref": "RGBA8", "ssim": ssim}
            row.update(alternate({"per_surface": loop, "batch": batch}, steps))
            print(json.dumps(row), flush=True)


def _fill(t, images):
    it = iter(images)
    for m in range(t.mip_level_count()):
        for f in range(t.face_count()):
            assert t.set_image(next(it), *((CubeFace(f), m) if t.face_count() == 6 else (m,)))
    return t


def compare_per_surface(t, source):
    """Texture.compare as it was before the batched entry: one Context.compare call per surface (block formats)"""
    mask = list(t.color_mask())
    if t.alpha_type() == api.Alpha.None_ or not Texture.has_alpha(t.format()):
        mask[3] = False
    ctx = t._context()
    results = [ctx.compare(p, source._images[m][d][f], t.format(), t.type(), mask=mask, ssim=True)
               for m, d, f, p in t._flat()]
    return results, Texture._pooled(results)


def batch_convert(steps, tile):
    chain = [im.astype(np.float32) / np.float32(255.0) for im in level_images(tile, 2048, 12)]
    cube = [im for im in level_images(tile, 1024, 11) for _ in range(6)]
    cases = [("2048^2 float32 chain -> BC7 Normal", Dimension.Dim2D, 2048, 12, chain, Format.BC7, Quality.Normal),
             ("1024^2 RGBA8 cube chain -> BC3 Normal", Dimension.Cube, 1024, 11, cube, Format.BC3, Quality.Normal)]
    for name, dim, size, mips, images, fmt, q in cases:
        source = _fill(Texture(dim, size, size, 0, mips), images)
        keep = Texture(dim, size, size, 0, mips)          # one context (and its staging) for every run
        keep._context()

        def fresh():
            t = _fill(Texture(dim, size, size, 0, mips), images)
            t._ctx = keep._ctx
            return t

        def two_calls():
            t = fresh()
            t0 = time.perf_counter()
            assert t.convert(fmt, Type.UNorm, q)
            compare_per_surface(t, source)
            return (time.perf_counter() - t0) * 1e3

        def two_calls_batched():
            t = fresh()
            t0 = time.perf_counter()
            assert t.convert(fmt, Type.UNorm, q)
            t.compare(source)
            return (time.perf_counter() - t0) * 1e3

        def one_call():
            t = fresh()
            t0 = time.perf_counter()
            assert t.convert_and_compare(fmt, Type.UNorm, q) is not None
            return (time.perf_counter() - t0) * 1e3
        row = {"row": "convert", "texture": name, "surfaces": len(images), "ssim": True, "unit": "wall ms"}
        row.update(alternate({"convert_then_per_surface_compare": two_calls, "convert_then_compare": two_calls_batched,
                              "convert_and_compare": one_call}, steps))
        print(json.dumps(row), flush=True)


def batch_transcode(steps, tile):
    images = level_images(tile, 4096, 13)
    t = _fill(Texture(Dimension.Dim2D, 4096, 4096, 0, 13), images)
    assert t.convert(Format.BC7, Type.UNorm, Quality.Lowest)

    def host(compare):
        t0 = time.perf_counter()
        out = t.transcode(Format.ASTC_6x6, Type.UNorm, Quality.Lowest)
        src = Texture(Dimension.Dim2D, 4096, 4096, 0, 13)
        src._ctx = t._ctx
        for m, level in enumerate(t.decode_images(api.PixelType.RGBA8)):
            assert src.set_image(level[0][0], m)
        compare(out, src)
        return (time.perf_counter() - t0) * 1e3

    def measured():
        t0 = time.perf_counter()
        assert t.transcode(Format.ASTC_6x6, Type.UNorm, Quality.Lowest, measure=True) is not None
        return (time.perf_counter() - t0) * 1e3
    row = {"row": "transcode", "texture": "BC7 -> ASTC 6x6, 4096^2 chain", "surfaces": 13, "ssim": True, "unit": "wall ms"}
    row.update(alternate({"transcode_then_per_surface_host_compare": lambda: host(compare_per_surface),
                          "transcode_then_host_compare": lambda: host(lambda out, src: out.compare(src)),
                          "transcode_measure": measured}, steps))
    print(json.dumps(row), flush=True)


def main_batch(args):
    dev = torch.device("cuda", 0)
    tile = synth.photo(TILE, TILE, seed=11)
    only = set(args.only.split(","))
    with Context(0) as ctx:
        if "single" in only:
            batch_single(ctx, args.steps, tile, dev)
        if "chains" in only:
            batch_chains(ctx, args.steps, tile)
    if "convert" in only:
        batch_convert(args.steps, tile)
    if "transcode" in only:
        batch_transcode(args.steps, tile)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--batch", action="store_true", help="measure the batched compare (DESIGN.md section 4.13)")
    ap.add_argument("--only", default="single,chains,convert,transcode")
    args = ap.parse_args()
    if args.batch:
        args.steps = 10 if args.steps is None else args.steps
        return main_batch(args)
    args.steps = 8 if args.steps is None else args.steps
    dev = torch.device("cuda", 0)
    tile = synth.photo(TILE, TILE, seed=11)
    tf = tile.astype(np.float32) / 255.0
    ref_np = np.tile(tf, (BIG // TILE, BIG // TILE, 1))
    ref = torch.from_numpy(ref_np).to(dev)
    ref_s = (ref * 2.0 - 1.0).contiguous()
    del ref_np
    res = torch.zeros(ctypes.sizeof(api.CompareResult), dtype=torch.uint8, device=dev)
    with Context(0) as ctx:
        for name, fmt, typ in ROWS:
            src = tf.astype(np.float16) if typ == 4 else (tf * 2.0 - 1.0 if typ == 1 else tile)
            p = ctx.encode([src], make_params(fmt, typ, Quality.Lowest))[0]
            pay = torch.from_numpy(tile_payload(p, fmt, typ, TILE, BIG)).to(dev)
            bw, bh, _ = api.query(fmt, typ)
            nblk = ((BIG + bw - 1) // bw) * ((BIG + bh - 1) // bh)
            emap = torch.empty(nblk, dtype=torch.float32, device=dev)
            r = ref_s if typ == 1 else ref
            layout, _ = api.decoded_layout(fmt, typ)
            torch.cuda.synchronize()

            def run(block_map, ssim):
                ctx.compare_device(pay.data_ptr(), fmt, typ, BIG, BIG, r.data_ptr(), api.PixelType.RGBA32F, BIG * 16,
                                   res.data_ptr(), ssim=ssim, block_errors=emap.data_ptr() if block_map else 0,
                                   block_errors_capacity=nblk if block_map else 0)
            base = pay.numel() + BIG * BIG * 16
            row = {"row": name, "format": Format(fmt).name, "type": Type(typ).name, "layout": layout.name,
                   "size": BIG, "ref": "RGBA32F", "bytes": base}
            for key, bm, ss in (("plain", False, False), ("map", True, False), ("ssim", False, True),
                                ("map_ssim", True, True)):
                ms = timed(ctx, lambda: run(bm, ss), args.steps)
                nbytes = base + (nblk * 4 if bm else 0)
                row[key + "_ms"] = round(ms, 4)
                row[key + "_frac_of_8TBps"] = round(nbytes / (ms * 1e-3) / HBM, 3)
            ch = api.LAYOUT_ARRAY[layout][0]
            row["bound_ms"] = round(base / HBM * 1e3, 4)
            if layout != api.Layout.RGBA16F:
                row["ssim_flop_per_texel"] = ssim_flops(ch)
                row["ssim_extra_ms"] = round(row["ssim_ms"] - row["plain_ms"], 4)
            print(json.dumps(row), flush=True)
            del pay, emap
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
