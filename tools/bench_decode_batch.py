#!/usr/bin/env python3
"""Batched decode (cfhip_decode_batch*) against the per-surface entries, one JSON line per case.

1. one 4096^2 surface, BC1 / BC7 / ASTC 6x6: cfhip_decode_batch_device against cfhip_decode_device, kernel time
   from the library's hipEvents on the launch stream (cfhip_last_kernel_ms), old and new alternating;
2. whole textures: decode_batch against a loop over decode on the same payloads, end to end (host clock around
   the synchronised calls) and summed kernel time (cfhip_profile_begin / _end);
3. RGBA32F against native output at 8192^2 for RGBA8 layouts, with the share of 8 TB/s from payload + output bytes;
4. Texture.transcode BC7 -> ASTC 6x6 Normal at 4096^2 with chain against save -> load -> decode_image loop -> convert.
Every figure: best and spread (max - min) of --repeats repeats after a warm-up.

    python tools/bench_decode_batch.py [--repeats 10] [--cases 1,2,3,4] [--out profiles/decode_batch.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import (Context, Dimension, FileType, Format, Quality, ResizeFilter, Texture, Type, api,  # noqa: E402
                            make_params, synth)

HBM = 8.0e12


def stat(v):
    return {"best": round(min(v), 4), "spread": round(max(v) - min(v), 4)}


def emit(fh, row):
    line = json.dumps(row)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def chain_sizes(n):
    return [(max(1, n >> l), max(1, n >> l)) for l in range(n.bit_length())]


def encode_chain(ctx, fmt, n, seed):
    """payloads of a full chain: level 0 encoded from a photo, the others from its top-left corner (content does
    not matter to a decoder's time)"""
    base = synth.photo(n, n, seed=seed)
    imgs = [np.ascontiguousarray(base[:h, :w]) for w, h in chain_sizes(n)]
    return ctx.encode(imgs, make_params(fmt, Type.UNorm, Quality.Lowest))


def case1(ctx, fh, reps):
    dev = torch.device("cuda", 0)
    img = synth.photo(4096, 4096, seed=11)
    for fmt in (Format.BC1_RGB, Format.BC7, Format.ASTC_6x6):
        pay = ctx.encode([img], make_params(fmt, Type.UNorm, Quality.Lowest))[0]
        d_pay = torch.from_numpy(pay).to(dev)
        d_out = torch.empty(4096*4096*4, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        surf = [dict(blocks=d_pay.data_ptr(), out=d_out.data_ptr(), width=4096, height=4096, out_pitch_bytes=4096*4)]
        old, new = [], []
        for i in range(reps + 2):
            ctx.decode_device(d_pay.data_ptr(), fmt, Type.UNorm, 4096, 4096, d_out.data_ptr(), 4096*4)
            a = ctx.last_kernel_ms()
            ctx.decode_batch_device(surf, fmt, Type.UNorm)
            b = ctx.last_kernel_ms()
            if i >= 2:
                old.append(a)
                new.append(b)
        emit(fh, {"case": 1, "format": fmt.name, "size": 4096, "per_surface_kernel_ms": stat(old),
                  "batched_kernel_ms": stat(new), "inside_per_surface_spread": abs(min(new) - min(old)) <= max(old) - min(old)})


def case2(ctx, fh, reps):
    jobs = [("BC7 4096 chain", Format.BC7, [encode_chain(ctx, Format.BC7, 4096, 3)], 4096),
            ("BC3 1024 cube chain", Format.BC3, [encode_chain(ctx, Format.BC3, 1024, 4 + f) for f in range(6)], 1024),
            ("ASTC 6x6 16 x 2048 chains", Format.ASTC_6x6, [encode_chain(ctx, Format.ASTC_6x6, 2048, 20)]*16, 2048)]
    for name, fmt, chains, n in jobs:
        pays = [p for c in chains for p in c]
        sizes = [s for _ in chains for s in chain_sizes(n)]

        def loop():
            return [ctx.decode(p, fmt, Type.UNorm, w, h) for p, (w, h) in zip(pays, sizes)]

        def batch():
            return ctx.decode_batch(pays, fmt, Type.UNorm, sizes)
        res = {}
        for _ in range(reps + 1):
            for key, fn in (("loop", loop), ("batch", batch)):
                ctx.profile_begin()
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0)*1e3
                kms, launches = ctx.profile_end()
                res.setdefault(key, []).append((ms, kms, launches))
        row = {"case": 2, "texture": name, "surfaces": len(pays)}
        for key in ("loop", "batch"):
            v = res[key][1:]
            row[key] = {"end_to_end_ms": stat([x[0] for x in v]), "kernel_ms": stat([x[1] for x in v]),
                        "launches": v[0][2]}
        emit(fh, row)


def case3(ctx, fh, reps):
    dev = torch.device("cuda", 0)
    n = 8192
    tile = synth.photo(4096, 4096, seed=11)
    for fmt in (Format.BC1_RGB, Format.BC7):
        p4 = ctx.encode([tile], make_params(fmt, Type.UNorm, Quality.Lowest))[0]
        bb = api.query(fmt, Type.UNorm)[2]
        pay = np.ascontiguousarray(np.tile(p4.reshape(1024, 1024, bb), (2, 2, 1))).reshape(-1)
        d_pay = torch.from_numpy(pay).to(dev)
        for pix, tb in ((None, 4), (api.PixelType.RGBA32F, 16)):
            d_out = torch.empty(n*n*tb, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            surf = [dict(blocks=d_pay.data_ptr(), out=d_out.data_ptr(), width=n, height=n, out_pitch_bytes=n*tb)]
            ms = []
            for i in range(reps + 2):
                ctx.decode_batch_device(surf, fmt, Type.UNorm, pix)
                if i >= 2:
                    ms.append(ctx.last_kernel_ms())
            nbytes = pay.nbytes + n*n*tb
            emit(fh, {"case": 3, "format": fmt.name, "size": n, "out": "native" if pix is None else pix.name,
                      "bytes": nbytes, "kernel_ms": stat(ms), "frac_of_8TBps": round(nbytes/(min(ms)*1e-3)/HBM, 3)})
            del d_out
            torch.cuda.empty_cache()


def case4(ctx, fh, reps):
    n = 4096
    t = Texture(Dimension.Dim2D, n, n)
    t.set_image(synth.photo(n, n, seed=5))
    t.generate_mipmaps(ResizeFilter.Box)
    t.convert(Format.BC7, Type.UNorm, Quality.Lowest)
    data = t.save_bytes(FileType.KTX)[1]
    reps = max(2, reps//3)

    def new():
        return Texture.load(data).transcode(Format.ASTC_6x6, Type.UNorm, Quality.Normal)

    def old():
        src = Texture.load(data)
        u = Texture(Dimension.Dim2D, n, n, 0, src.mip_level_count())
        for m in range(src.mip_level_count()):
            u.set_image(src.decode_image(m), m)
        u.convert(Format.ASTC_6x6, Type.UNorm, Quality.Normal)
        return u
    res = {"old": [], "new": []}
    same = None
    for i in range(reps + 1):
        for key, fn in (("old", old), ("new", new)):
            t0 = time.perf_counter()
            r = fn()
            res[key].append((time.perf_counter() - t0)*1e3)
            if key == "old":
                keep = r
            else:
                same = all(np.array_equal(r.data(m), keep.data(m)) for m in range(r.mip_level_count()))
    emit(fh, {"case": 4, "what": "BC7 -> ASTC 6x6 Normal, 4096 chain", "host_route_ms": stat(res["old"][1:]),
              "transcode_ms": stat(res["new"][1:]), "same_bytes": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cases", default="1,2,3,4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fh = open(args.out, "w") if args.out else None
    with Context(0) as ctx:
        for c, fn in ((1, case1), (2, case2), (3, case3), (4, case4)):
            if str(c) in args.cases.split(","):
                fn(ctx, fh, args.repeats)


if __name__ == "__main__":
    main()
