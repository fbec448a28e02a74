#!/usr/bin/env python3
"""Kernel time of the zlib encoder (csrc/deflate.hip) beside the estimator on the same bytes
and zlib on the host, one JSON line per row.

Input and rows: those of tools/bench_lzsize.py -- synth.photo seed 1, a 1024^2 tile repeated to --size^2, encoded at
Quality.Normal to BC7 (16 MiB at 4096^2) and BC1 (8 MiB); each plain and after the pass (Context.rdo_device at the row's
lambda).  Per row: Context.deflate_device on the resident payload, best of --steps runs after a warm-up with spread =
max - min; total_ms is cfhip_last_kernel_ms (hipEvents around every stage of every slice), stage_ms the eight stages of
the best run (cfhip_deflate_stage_ms), wall_ms the host clock around the blocking call.  Then Context.lz_size_device on
the same bytes the same way, zlib.compress at levels 1 and 9 on this host (size and seconds, one run each), the
ratios, and a check that zlib reads the stream back.

    python tools/bench_deflate.py [--steps 5] [--size 4096] [--out profiles/deflate_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth  # noqa: E402

ROWS = [(Format.BC7, 2.0), (Format.BC1_RGB, 4.0)]
TILE = 1024
ONE_LANE = ("parse", "codes", "offsets")       # the stages with a part that one lane runs


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.size
    reps = (n + TILE - 1)//TILE
    img = np.ascontiguousarray(np.tile(synth.photo(TILE, TILE, seed=1), (reps, reps, 1))[:n, :n])
    tex = torch.from_numpy(img).to(dev)
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    with Context(0) as ctx:
        for fmt, lam in ROWS:
            nbytes = api.payload_size(fmt, Type.UNorm, n, n)
            cap = api.deflate_bound(nbytes)
            plain = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            work = torch.empty_like(plain)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            rstats = torch.zeros(ctypes.sizeof(api.RdoStats), dtype=torch.uint8, device=dev)
            lstats = torch.zeros(ctypes.sizeof(api.LzStats), dtype=torch.uint8, device=dev)
            dres = torch.zeros(ctypes.sizeof(api.DeflateResult), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.encode_device([dict(pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4,
                                    out=plain.data_ptr(), out_capacity=nbytes)], make_params(fmt, Type.UNorm, Quality.Normal))
            ctx.rdo_device([dict(blocks=plain.data_ptr(), out=work.data_ptr(), out_capacity=nbytes, pixels=tex.data_ptr(),
                                 pixel_type=0, width=n, height=n, row_pitch_bytes=n*4)], fmt, Type.UNorm, lam,
                           rstats.data_ptr())
            for what, buf in (("plain", plain), ("rdo lambda %g" % lam, work)):
                runs, est = [], []
                for step in range(args.steps + 1):
                    _, wall = timed(lambda: ctx.deflate_device([(buf.data_ptr(), nbytes)], out.data_ptr(), cap,
                                                               dres.data_ptr()))
                    if step:                                       # step 0 warms up
                        runs.append((ctx.last_kernel_ms(), wall*1e3, ctx.deflate_stage_ms()))
                for step in range(args.steps + 1):
                    ctx.lz_size_device([(buf.data_ptr(), nbytes)], lstats.data_ptr())
                    if step:
                        est.append(ctx.last_kernel_ms())
                res = api.DeflateResult.from_buffer_copy(dres.cpu().numpy().tobytes()).as_dict()
                st = api.LzStats.from_buffer_copy(lstats.cpu().numpy().tobytes()).as_dict()
                host = buf.cpu().numpy().tobytes()
                stream = out[:res["bytes_out"]].cpu().numpy().tobytes()
                back, inflate_s = timed(lambda: zlib.decompress(stream))
                z9, s9 = timed(lambda: len(zlib.compress(host, 9)))
                z1, s1 = timed(lambda: len(zlib.compress(host, 1)))
                best = min(runs, key=lambda r: r[0])
                stages = best[2]
                emit({"row": "deflate", "format": fmt.name, "payload": what, "size": n, "bytes": nbytes, "steps": args.steps,
                      "total_ms_best": round(best[0], 4), "total_ms_spread": round(max(r[0] for r in runs) - best[0], 4),
                      "wall_ms_best": round(min(r[1] for r in runs), 3),
                      "stage_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stage_share": {k: round(v/best[0], 3) for k, v in stages.items()},
                      "one_lane_stages_share": round(sum(stages[k] for k in ONE_LANE)/best[0], 3),
                      "gbytes_per_s": round(nbytes/best[0]/1e6, 3), "result": res, "round_trip": back == host,
                      "lz_size_ms_best": round(min(est), 4), "over_lz_size": round(best[0]/min(est), 3),
                      "est_bytes": st["est_bytes"], "stream_over_estimate": round(res["bytes_out"]/st["est_bytes"], 4),
                      "zlib9_bytes": z9, "zlib9_s": round(s9, 3), "zlib1_bytes": z1, "zlib1_s": round(s1, 3),
                      "stream_over_zlib9": round(res["bytes_out"]/z9, 4), "stream_over_zlib1": round(res["bytes_out"]/z1, 4),
                      "zlib9_over_kernel_time": round(s9*1e3/best[0], 1), "zlib1_over_kernel_time": round(s1*1e3/best[0], 1),
                      "zlib9_over_wall_time": round(s9*1e3/min(r[1] for r in runs), 1),
                      "zlib1_over_wall_time": round(s1*1e3/min(r[1] for r in runs), 1)})
            del plain, work, out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
