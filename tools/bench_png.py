#!/usr/bin/env python3
"""The PNG writer (csrc/png.hip): what it costs in size (--ratio, on the CPU) and what it takes in
time (on the GPU), beside a host writer and beside the zlib encoder alone on the same bytes.

--ratio: the twin (tests/png_ref.py, whose bytes the GPU writes exactly) against Pillow's save(format="PNG",
compress_level=9) as RGB8 on the six crops of tests/golden/pvrtc_photos.npz and synth.photo(256, 256, seed=1): the
images the size guard of tests/test_png_ref.py asserts.  Prints markdown; --out writes it.

Time (the default): synth.photo seed 1, a 1024^2 tile repeated to 4096^2 and 8192^2 as RGBA8 at depth 8, and to 4096^2 as
RGBA32F at depth 16, resident in HBM.  Per row: png_encode_device, --steps runs after a warm-up, the minimum and the
spread (max - min) of cfhip_last_kernel_ms (hipEvents around every stage) and the stages of the best run; then, in the
same run, deflate_device alone on the same filtered bytes (the file's own IDAT data inflated and uploaded), and Pillow's
save at compress_level 6 and 1 on this host by the host clock (8-bit rows: Pillow has no 16-bit RGBA).  The 8-bit files
are opened with Pillow and compared with the source.  One JSON line per row, appended to --out.

    python tools/bench_png.py --ratio [--out profiles/png_ratio.md]
    python tools/bench_png.py [--steps 5] [--out profiles/png_bench.jsonl]
"""
import argparse
import io
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def ratio(args):
    from PIL import Image

    import png_ref as P
    from test_png_ref import pillow_bytes, ratio_images
    lines = ["# The PNG files against Pillow (CPU twin)", "",
             "`tools/bench_png.py --ratio`.  twin: the file of `tests/png_ref.py`, which the GPU writes exactly (the",
             "specification's filter heuristic per row, one zlib stream of `tests/deflate_ref.py`: 64 KiB groups, four",
             "candidates, 32 KiB window).  Pillow 9 / 6 / 1: `save(format=\"PNG\", compress_level=...)`, libpng's own",
             "filter choice over zlib.  All as RGB8.  ratio: twin / Pillow 9, what the size guard of",
             "`tests/test_png_ref.py` bounds.  rows: per filter type None, Sub, Up, Average, Paeth.", "",
             "| image | size | raw bytes | Pillow 9 | Pillow 6 | Pillow 1 | twin | ratio | rows |",
             "|---|---|---|---|---|---|---|---|---|"]
    ratios = []
    for name, img in ratio_images():
        data, res = P.encode(img, P.RGB, 8)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img[..., :3])
        p9, p6, p1 = (pillow_bytes(img, level) for level in (9, 6, 1))
        ratios.append(len(data)/p9)
        lines.append("| %s | %dx%d | %d | %d | %d | %d | %d | %.4f | %s |" % (
            name, img.shape[1], img.shape[0], img.shape[0]*img.shape[1]*3, p9, p6, p1, len(data), ratios[-1],
            ", ".join(str(v) for v in res["rows_by_filter"])))
    lines += ["", "twin / Pillow 9 over the %d images: %.4f ... %.4f." % (len(ratios), min(ratios), max(ratios))]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def best_of(runs):
    best = min(runs, key=lambda r: r[0])
    return best, round(max(r[0] for r in runs) - best[0], 4)


def timing(args):
    import torch
    from PIL import Image

    import png_ref as P
    from cuttlefish_amd import Context, api, synth
    dev = torch.device("cuda", 0)
    tile = synth.photo(1024, 1024, seed=1)
    rows = [(4096, np.uint8, 8), (8192, np.uint8, 8), (4096, np.float32, 16)]
    if args.size:
        rows = [r for r in rows if r[0] == args.size]
    with Context(0) as ctx:
        for n, dt, depth in rows:
            host = np.tile(tile, (n//1024, n//1024, 1))
            if dt != np.uint8:
                host = (host.astype(np.float32)/np.float32(255.0)).astype(dt)
            tb = 4*host.dtype.itemsize
            src = torch.from_numpy(host.view(np.uint8).reshape(n, n*tb) if dt != np.uint8 else host.reshape(n, n*4)).to(dev)
            cap = api.png_bound(n, n, api.PNG_RGBA, depth)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            res = torch.zeros(15, dtype=torch.int64, device=dev)

            def encode():
                ctx.png_encode_device(src.data_ptr(), api.pixel_type_of(host), n*tb, n, n, out.data_ptr(), cap, res.data_ptr(),
                                      color_type=api.PNG_RGBA, bit_depth=depth)
                return ctx.last_kernel_ms(), ctx.png_stage_ms()
            encode()
            (ms, stages), spread = best_of([encode() for _ in range(args.steps)])
            r = api.PngResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
            data = out[:r["bytes_out"]].cpu().numpy().tobytes()
            chunks = P.read_chunks(data)                           # every CRC
            filtered = zlib.decompress(chunks[-2][1])
            assert len(filtered) == r["filtered_bytes"] == n*(1 + n*4*depth//8)
            # the zlib encoder alone on the same bytes
            fbytes = torch.from_numpy(np.frombuffer(filtered, np.uint8).copy()).to(dev)
            zcap = api.deflate_bound(len(filtered))
            zout = torch.empty(zcap, dtype=torch.uint8, device=dev)
            zres = torch.zeros(9, dtype=torch.int64, device=dev)

            def deflate():
                ctx.deflate_device([(fbytes.data_ptr(), len(filtered))], zout.data_ptr(), zcap, zres.data_ptr())
                return (ctx.last_kernel_ms(),)
            deflate()
            (dms,), dspread = best_of([deflate() for _ in range(args.steps)])
            row = {"bench": "png", "size": n, "source": host.dtype.name, "bit_depth": depth, "source_bytes": int(host.nbytes),
                   "filtered_bytes": r["filtered_bytes"], "file_bytes": r["bytes_out"], "rows_by_filter": r["rows_by_filter"],
                   "kernel_ms": round(ms, 4), "spread_ms": spread, "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                   "filter_gb_s": round((2*host.nbytes + r["filtered_bytes"])/stages["filter"]/1e6, 1),
                   "crc_gb_s": round(r["idat_bytes"]/stages["crc"]/1e6, 1),
                   "deflate_alone_ms": round(dms, 4), "deflate_alone_spread_ms": dspread, "steps": args.steps}
            if depth == 8:
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), host)
                row["pillow_reads_exact"] = True
                pil = Image.fromarray(host)
                for level in (6, 1):
                    b = io.BytesIO()
                    t0 = time.perf_counter()
                    pil.save(b, format="PNG", compress_level=level)
                    row["pillow_%d_ms" % level] = round((time.perf_counter() - t0)*1e3, 1)
                    row["pillow_%d_bytes" % level] = len(b.getvalue())
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del src, out, fbytes, zout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=0, help="only the rows of this size")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ratio:
        ratio(args)
    else:
        timing(args)


if __name__ == "__main__":
    main()
