#!/usr/bin/env python3
"""Kernel time of the rate-distortion pass (csrc/rdo.hip) at 4096^2 against the same
format's Quality.Normal encode kernel, one JSON line per (format, input).

Inputs: synth.photo seed 1 and synth.photo2, 1024^2 tiles repeated to 4096^2, RGBA8, resident on the device.  Per
row the encode (Context.encode_device, Normal) and the pass (Context.rdo_device on the fresh payload, out of place
so that every run reads the same input) alternate in one process; each figure is the best of --steps runs after a
warm-up round, with spread = max - min.  Times are cfhip_last_kernel_ms (hipEvents around the launch).  ratio =
rdo_best / encode_best.  The row also carries the pass's statistics and the library's segment length, so that rows
of libraries built with another CFRDO_SEG (CFHIP_LIB=...) can be told apart: pass --seg to label them.

--row-above adds the pass with copies from the block row above (cfhip_rdo2d_kernel) as a third kernel of the
alternation: rdo2d_ms_best / _spread, its ratio to the plain pass and to the encode, and its statistics.  Label a
library built with another CFRDO_TILE_ROWS with --tile-rows.

    python tools/bench_rdo.py [--steps 8] [--size 4096] [--seg 64] [--row-above [--tile-rows 8]]
                              [--out profiles/rdo_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth  # noqa: E402

# format -> lambda: the middle of the range profiles/rdo_quality.md covers
ROWS = [(Format.BC1_RGB, 4.0), (Format.BC3, 4.0), (Format.BC7, 2.0)]
TILE = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--seg", type=int, default=64, help="label: CFRDO_SEG of the library under test")
    ap.add_argument("--row-above", action="store_true", help="also time the pass with copies from the row above")
    ap.add_argument("--tile-rows", type=int, default=8, help="label: CFRDO_TILE_ROWS of the library under test")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdo_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.size
    inputs = [("photo seed 1", synth.photo(TILE, TILE, seed=1)), ("photo2", synth.photo2(TILE, TILE))]
    size = ctypes.sizeof(api.RdoStats)
    lines = []
    with Context(0) as ctx:
        for name, tile in inputs:
            reps = (n + TILE - 1)//TILE
            img = np.ascontiguousarray(np.tile(tile, (reps, reps, 1))[:n, :n])
            tex = torch.from_numpy(img).to(dev)
            for fmt, lam in ROWS:
                nbytes = api.payload_size(fmt, Type.UNorm, n, n)
                pay = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                out = torch.empty_like(pay)
                stats = torch.zeros(size, dtype=torch.uint8, device=dev)
                params = make_params(fmt, Type.UNorm, Quality.Normal)
                enc_surface = [dict(pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4,
                                    out=pay.data_ptr(), out_capacity=nbytes)]
                rdo_surface = [dict(blocks=pay.data_ptr(), out=out.data_ptr(), out_capacity=nbytes,
                                    pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4)]

                def encode():
                    ctx.encode_device(enc_surface, params)
                    return ctx.last_kernel_ms()

                def rdo():
                    ctx.rdo_device(rdo_surface, fmt, Type.UNorm, lam, stats.data_ptr())
                    return ctx.last_kernel_ms()

                def rdo2d():
                    ctx.rdo_device(rdo_surface, fmt, Type.UNorm, lam, stats.data_ptr(), row_above=True)
                    return ctx.last_kernel_ms()
                torch.cuda.synchronize()                          # torch's fills run on its own stream
                kernels = {"encode": encode, "rdo": rdo}
                if args.row_above:
                    kernels["rdo2d"] = rdo2d
                for k in kernels.values():                        # warm-up round
                    k()
                runs = {name: [] for name in kernels}
                for _ in range(args.steps):
                    for name, k in kernels.items():
                        runs[name].append(k())
                if args.row_above:
                    st2d = api.RdoStats.from_buffer_copy(stats.cpu().numpy().tobytes()).as_dict()
                    rdo()
                st = api.RdoStats.from_buffer_copy(stats.cpu().numpy().tobytes()).as_dict()
                row = {"format": fmt.name, "input": name, "size": n, "lambda": lam, "seg": args.seg, "steps": args.steps,
                       "encode_normal_ms_best": round(min(runs["encode"]), 4),
                       "encode_normal_ms_spread": round(max(runs["encode"]) - min(runs["encode"]), 4),
                       "rdo_ms_best": round(min(runs["rdo"]), 4),
                       "rdo_ms_spread": round(max(runs["rdo"]) - min(runs["rdo"]), 4)}
                row["ratio"] = round(row["rdo_ms_best"]/row["encode_normal_ms_best"], 3)
                row["gblocks_per_s"] = round(st["blocks"]/(row["rdo_ms_best"]*1e-3)/1e9, 3)
                row["stats"] = st
                if args.row_above:
                    row.update({"tile_rows": args.tile_rows, "rdo2d_ms_best": round(min(runs["rdo2d"]), 4),
                                "rdo2d_ms_spread": round(max(runs["rdo2d"]) - min(runs["rdo2d"]), 4), "stats_2d": st2d})
                    row["rdo2d_over_rdo"] = round(row["rdo2d_ms_best"]/row["rdo_ms_best"], 3)
                    row["rdo2d_over_encode"] = round(row["rdo2d_ms_best"]/row["encode_normal_ms_best"], 3)
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
                del pay, out
            del tex
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
