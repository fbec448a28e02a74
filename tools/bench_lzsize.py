#!/usr/bin/env python3
"""Kernel time of the deflate-size estimator (csrc/lzsize.hip) and of the search built on it,
beside zlib on the host, one JSON line per row.

Input: synth.photo seed 1, a 1024^2 tile repeated to --size^2, RGBA8, resident on the device; encoded at
Quality.Normal to BC7 (16 MiB at 4096^2) and BC1 (8 MiB).  Per format:

  * "estimate" rows, for the plain payload and for the one after the pass (Context.rdo_device at the row's lambda):
    Context.lz_size_device on the resident payload, best of --steps runs after a warm-up with spread = max - min;
    total_ms is cfhip_last_kernel_ms (hipEvents around every stage of every slice), stage_ms the five stages of the
    best run (cfhip_lz_stage_ms), wall_ms the host clock around the blocking call.  Beside them zlib.compress at
    levels 9 and 1 on the same bytes on this host: size and seconds, one run each, and estimate / zlib-9.
  * a "target" row: Context.rdo_target_device to --ratio under a ceiling of lambda 32, in place: wall seconds, summed
    kernel ms of all trials, the result; and, with --zlib-loop, the same bisection with the pass on the device and
    zlib-9 on the host as the size function.

    python tools/bench_lzsize.py [--steps 5] [--size 4096] [--ratio 0.85] [--zlib-loop] [--out profiles/lzsize_bench.jsonl]
"""
import argparse
import ctypes
import json
import math
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
CEILING = 32.0


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ratio", type=float, default=0.85)
    ap.add_argument("--zlib-loop", action="store_true", help="also run the bisection with zlib-9 as the size function")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lzsize_bench.jsonl"))
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
            plain = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            work = torch.empty_like(plain)
            rstats = torch.zeros(ctypes.sizeof(api.RdoStats), dtype=torch.uint8, device=dev)
            lstats = torch.zeros(ctypes.sizeof(api.LzStats), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.encode_device([dict(pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4,
                                    out=plain.data_ptr(), out_capacity=nbytes)], make_params(fmt, Type.UNorm, Quality.Normal))
            surface = dict(blocks=plain.data_ptr(), out=work.data_ptr(), out_capacity=nbytes, pixels=tex.data_ptr(),
                           pixel_type=0, width=n, height=n, row_pitch_bytes=n*4)

            def run_pass(lam_):
                ctx.rdo_device([surface], fmt, Type.UNorm, lam_, rstats.data_ptr())
                return ctx.last_kernel_ms()
            rdo_ms = run_pass(lam)
            for what, buf in (("plain", plain), ("rdo lambda %g" % lam, work)):
                runs = []
                for step in range(args.steps + 1):
                    _, wall = timed(lambda: ctx.lz_size_device([(buf.data_ptr(), nbytes)], lstats.data_ptr()))
                    if step:                                       # step 0 warms up
                        runs.append((ctx.last_kernel_ms(), wall*1e3, ctx.lz_stage_ms()))
                st = api.LzStats.from_buffer_copy(lstats.cpu().numpy().tobytes()).as_dict()
                host = buf.cpu().numpy().tobytes()
                z9, s9 = timed(lambda: len(zlib.compress(host, 9)))
                z1, s1 = timed(lambda: len(zlib.compress(host, 1)))
                best = min(runs, key=lambda r: r[0])
                emit({"row": "estimate", "format": fmt.name, "payload": what, "size": n, "bytes": nbytes, "steps": args.steps,
                      "total_ms_best": round(best[0], 4), "total_ms_spread": round(max(r[0] for r in runs) - best[0], 4),
                      "wall_ms_best": round(min(r[1] for r in runs), 3),
                      "stage_ms": {k: round(v, 4) for k, v in best[2].items()}, "gbytes_per_s": round(nbytes/best[0]/1e6, 3),
                      "stats": st, "zlib9_bytes": z9, "zlib9_s": round(s9, 3), "zlib1_bytes": z1, "zlib1_s": round(s1, 3),
                      "estimate_over_zlib9": round(st["est_bytes"]/z9, 4), "rdo_pass_ms": round(rdo_ms, 4)})
            # the search, in place on a copy of the plain payload
            in_place = dict(surface, blocks=work.data_ptr())
            walls = []
            for step in range(2):
                work.copy_(plain)
                torch.cuda.synchronize()
                res, wall = timed(lambda: ctx.rdo_target_device([in_place], fmt, Type.UNorm, args.ratio, CEILING,
                                                                rstats.data_ptr()))
                walls.append((wall, ctx.last_kernel_ms()))
            row = {"row": "target", "format": fmt.name, "size": n, "bytes": nbytes, "ratio": args.ratio, "ceiling": CEILING,
                   "wall_s_best": round(min(w for w, _ in walls), 4), "kernel_ms": round(min(k for _, k in walls), 3),
                   "result": res}
            if args.zlib_loop:
                host_plain = plain.cpu().numpy().tobytes()

                def zsize(lam16):
                    run_pass(lam16/16.0)
                    return len(zlib.compress(work.cpu().numpy().tobytes(), 9))

                def bisect():
                    target = math.floor(float(np.float32(args.ratio))*len(zlib.compress(host_plain, 9)))
                    hi, lo, trials = int(round(16*CEILING)), 0, 1
                    reached = zsize(hi) <= target
                    while reached and hi - lo > 1:
                        mid = (lo + hi)//2
                        trials += 1
                        if zsize(mid) <= target:
                            hi = mid
                        else:
                            lo = mid
                    return dict(lambda16=hi, reached=int(reached), trials=trials)
                zres, zwall = timed(bisect)
                row.update({"zlib9_loop_s": round(zwall, 2), "zlib9_loop_result": zres})
            emit(row)
            del plain, work
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
