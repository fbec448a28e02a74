#!/usr/bin/env python3
"""Kernel time of the indexed inflater (csrc/inflate.hip) beside what a user does without it --
zlib.decompress of the same stream on this host plus the upload of the result -- and beside the encoder on the same
bytes, one JSON line per row.

Input and rows: those of tools/bench_deflate.py -- synth.photo seed 1, a 1024^2 tile repeated to --size^2, encoded at
Quality.Normal to BC7 (16 MiB at 4096^2) and BC1 (8 MiB); each plain and after the pass (Context.rdo_device at the row's
lambda).  Per row: Context.deflate_indexed_device on the resident payload, then Context.inflate_device of that stream
and index, best of --steps runs after a warm-up with spread = max - min; total_ms is cfhip_last_kernel_ms (hipEvents
around every stage of every slice), stage_ms the four stages of the best run (cfhip_inflate_stage_ms), wall_ms the
host clock around the blocking call; `rounds`; the bytes compared with the payload on the device.  The yardstick:
zlib.decompress (best of --steps) and the upload of its result (torch, from pageable memory, best of --steps).

    python tools/bench_inflate.py [--steps 5] [--size 4096] [--out profiles/inflate_bench.jsonl]
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


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.jsonl"))
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
            cap, entries = api.deflate_bound(nbytes), api.zindex_entries(nbytes)
            plain = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            work = torch.empty_like(plain)
            back = torch.empty_like(plain)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            index = torch.zeros((entries, 2), dtype=torch.int64, device=dev)
            rstats = torch.zeros(ctypes.sizeof(api.RdoStats), dtype=torch.uint8, device=dev)
            dres = torch.zeros(ctypes.sizeof(api.DeflateResult), dtype=torch.uint8, device=dev)
            ires = torch.zeros(ctypes.sizeof(api.InflateResult), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.encode_device([dict(pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4,
                                    out=plain.data_ptr(), out_capacity=nbytes)], make_params(fmt, Type.UNorm, Quality.Normal))
            ctx.rdo_device([dict(blocks=plain.data_ptr(), out=work.data_ptr(), out_capacity=nbytes, pixels=tex.data_ptr(),
                                 pixel_type=0, width=n, height=n, row_pitch_bytes=n*4)], fmt, Type.UNorm, lam,
                           rstats.data_ptr())
            for what, buf in (("plain", plain), ("rdo lambda %g" % lam, work)):
                enc, runs = [], []
                for step in range(args.steps + 1):
                    ctx.deflate_indexed_device([(buf.data_ptr(), nbytes)], out.data_ptr(), cap, index.data_ptr(), entries,
                                               dres.data_ptr())
                    if step:                                       # step 0 warms up
                        enc.append(ctx.last_kernel_ms())
                dr = api.DeflateResult.from_buffer_copy(dres.cpu().numpy().tobytes()).as_dict()
                for step in range(args.steps + 1):
                    back.zero_()
                    torch.cuda.synchronize()
                    _, wall = timed(lambda: ctx.inflate_device(out.data_ptr(), dr["bytes_out"], index.data_ptr(), entries,
                                                               back.data_ptr(), nbytes, ires.data_ptr()))
                    if step:
                        runs.append((ctx.last_kernel_ms(), wall*1e3, ctx.inflate_stage_ms()))
                res = api.InflateResult.from_buffer_copy(ires.cpu().numpy().tobytes()).as_dict()
                same = bool((back == buf).all())
                stream = out[:dr["bytes_out"]].cpu().numpy().tobytes()
                host_s, up_s, raw = [], [], b""
                for _ in range(args.steps):
                    raw, s = timed(lambda: zlib.decompress(stream))
                    host_s.append(s)
                    arr = np.frombuffer(raw, np.uint8).copy()       # writable, as torch wants it; not timed
                    torch.cuda.synchronize()
                    _, s = timed(lambda: (torch.from_numpy(arr).to(dev), torch.cuda.synchronize()))
                    up_s.append(s)
                best = min(runs, key=lambda r: r[0])
                stages = best[2]
                host_ms = (min(host_s) + min(up_s))*1e3
                emit({"row": "inflate", "format": fmt.name, "payload": what, "size": n, "bytes": nbytes, "steps": args.steps,
                      "stream_bytes": dr["bytes_out"], "index_bytes": entries*16,
                      "total_ms_best": round(best[0], 4), "total_ms_spread": round(max(r[0] for r in runs) - best[0], 4),
                      "wall_ms_best": round(min(r[1] for r in runs), 3),
                      "stage_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stage_share": {k: round(v/best[0], 3) for k, v in stages.items()},
                      "out_gbytes_per_s": round(nbytes/best[0]/1e6, 3), "rounds": res["rounds"], "result": res,
                      "round_trip": same and raw == buf.cpu().numpy().tobytes(),
                      "zlib_decompress_ms": round(min(host_s)*1e3, 3), "upload_ms": round(min(up_s)*1e3, 3),
                      "host_over_kernel_time": round(host_ms/best[0], 2),
                      "host_over_wall_time": round(host_ms/min(r[1] for r in runs), 2),
                      "deflate_ms_best": round(min(enc), 4), "over_deflate": round(best[0]/min(enc), 3)})
            del plain, work, back, out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
