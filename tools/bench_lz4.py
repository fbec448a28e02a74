#!/usr/bin/env python3
"""The LZ4 frame codec (csrc/lz4.hip): what it costs in size (--ratio, on the CPU) and what it
takes in time (on the GPU), beside the zlib path on the same bytes.

--ratio: the twin (tests/lz4_ref.py, whose bytes the GPU writes exactly) against liblz4's LZ4_compress_default and
LZ4_compress_HC level 9, both per independent 64 KiB block and framed the same way (19 bytes + 8 per block, a block
that does not shrink stored), and against zlib level 9, on the 32 payload rows of tests/lzsize_cases.py (oracle payloads
at Quality.Normal of two photographic inputs for ten formats, BC1 / BC7 also after rdo_ref at three lambdas), and on the
two cases the size guard of tests/test_lz4_ref.py asserts.  Needs liblz4.so.1.  Prints markdown; --out writes it.

Time (the default): synth.photo seed 1, a 1024^2 tile repeated to --size^2, encoded at Quality.Normal to BC7 (16 MiB at
4096^2) and BC1 (8 MiB), each plain and after the pass (Context.rdo_device).  Per row, on the resident payload:
lz4_encode_device and lz4_decode_device, then deflate_indexed_device and inflate_device of the same bytes in the same
run; each --steps runs after a warm-up, the minimum and the spread (max - min) of cfhip_last_kernel_ms (hipEvents around
every stage) and the stages of the best run.  Where liblz4 is present: LZ4F_decompress of our frame on this host plus
the upload of the result, by the host clock.  One JSON line per row, appended to --out.

    python tools/bench_lz4.py --ratio [--out profiles/lz4_ratio.md]
    python tools/bench_lz4.py [--steps 5] [--size 4096] [--out profiles/lz4_bench.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

BLOCK = 65536


def liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    lib.LZ4_compressBound.argtypes = [ctypes.c_int]
    lib.LZ4_compress_default.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_compress_HC.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    lib.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.LZ4F_decompress.restype = ctypes.c_size_t
    lib.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lib.LZ4F_isError.argtypes = [ctypes.c_size_t]
    return lib


def framed(lib, raw: bytes, level):
    """bytes of a frame like ours whose blocks liblz4 compressed: level None = LZ4_compress_default, else LZ4_compress_HC"""
    total = 19
    for s in range(0, len(raw), BLOCK):
        blk = raw[s:s + BLOCK]
        cap = lib.LZ4_compressBound(len(blk))
        out = ctypes.create_string_buffer(cap)
        c = lib.LZ4_compress_default(blk, out, len(blk), cap) if level is None else \
            lib.LZ4_compress_HC(blk, out, len(blk), cap, level)
        assert c > 0
        total += 8 + min(c, len(blk))
    return total


def ratio(args):
    import deflate_cases
    import lz4_cases
    import lz4_ref as R
    import lzsize_cases as C
    lib = liblz4()
    if lib is None:
        sys.exit("liblz4.so.1 is absent")
    rows = [(name, p.tobytes()) for name, p in C.payload_rows()]
    guard = [("guard: BC1 rdo 32768", lz4_cases.content("BC1 rdo", 32768).tobytes()),
             ("guard: text 204800", lz4_cases.content("text", deflate_cases.BIG).tobytes())]
    lines = ["# The LZ4 frames against liblz4 and zlib (CPU twin)", "",
             "`tools/bench_lz4.py --ratio`.  twin: the frame of `tests/lz4_ref.py`, which the GPU writes exactly (lazy parse,",
             "four candidates, 32 KiB window, 4 KiB chunks).  default / HC 9: `LZ4_compress_default` / `LZ4_compress_HC` level 9",
             "of liblz4 per independent 64 KiB block, framed like the twin's.  Fractions are of the raw size.  excess:",
             "(twin - default) / raw, what the size guard of `tests/test_lz4_ref.py` bounds.", "",
             "| payload | bytes | zlib-9 | default | HC 9 | twin | excess | compressed, stored | sequences |",
             "|---|---|---|---|---|---|---|---|---|"]
    excess, between = [], 0
    for name, raw in rows + guard:
        n = len(raw)
        frame, res = R.encode(np.frombuffer(raw, np.uint8))
        assert R.decode(frame, n)[0] == raw
        d, h, z = framed(lib, raw, None), framed(lib, raw, 9), len(zlib.compress(raw, 9))
        if not name.startswith("guard"):
            excess.append((len(frame) - d)/n)
            between += h <= len(frame) <= d
        lines.append("| %s | %d | %.4f | %.4f | %.4f | %.4f | %+.4f | %d, %d | %d |" % (
            name, n, z/n, d/n, h/n, len(frame)/n, (len(frame) - d)/n, res["blocks_compressed"], res["blocks_stored"],
            res["sequences"]))
    lines += ["", "Over the 32 payload rows: excess %+.4f ... %+.4f of the raw size; the twin lies between HC 9 and default on %d of %d."
              % (min(excess), max(excess), between, len(excess))]
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

    from cuttlefish_amd import Context, Format, Quality, Type, api, make_params, synth
    lib = liblz4()
    dev = torch.device("cuda", 0)
    n, tile = args.size, 1024
    reps = (n + tile - 1)//tile
    img = np.ascontiguousarray(np.tile(synth.photo(tile, tile, seed=1), (reps, reps, 1))[:n, :n])
    tex = torch.from_numpy(img).to(dev)
    lines = []
    with Context(0) as ctx:
        for fmt, lam in ((Format.BC7, 2.0), (Format.BC1_RGB, 4.0)):
            nbytes = api.payload_size(fmt, Type.UNorm, n, n)
            plain = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            work = torch.empty_like(plain)
            back = torch.empty_like(plain)
            lcap, zcap, entries = api.lz4_bound(nbytes), api.deflate_bound(nbytes), api.zindex_entries(nbytes)
            lout = torch.empty(lcap, dtype=torch.uint8, device=dev)
            zout = torch.empty(zcap, dtype=torch.uint8, device=dev)
            zidx = torch.empty((entries, 2), dtype=torch.int64, device=dev)
            res = torch.zeros(256, dtype=torch.uint8, device=dev)
            rstats = torch.zeros(ctypes.sizeof(api.RdoStats), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.encode_device([dict(pixels=tex.data_ptr(), pixel_type=0, width=n, height=n, row_pitch_bytes=n*4,
                                    out=plain.data_ptr(), out_capacity=nbytes)], make_params(fmt, Type.UNorm, Quality.Normal))
            ctx.rdo_device([dict(blocks=plain.data_ptr(), out=work.data_ptr(), out_capacity=nbytes, pixels=tex.data_ptr(),
                                 pixel_type=0, width=n, height=n, row_pitch_bytes=n*4)], fmt, Type.UNorm, lam,
                           rstats.data_ptr())

            def result(cls):
                return cls.from_buffer_copy(res.cpu().numpy().tobytes()[:ctypes.sizeof(cls)]).as_dict()
            for what, buf in (("plain", plain), ("rdo lambda %g" % lam, work)):
                enc, dec, zenc, zdec = [], [], [], []
                for step in range(args.steps + 1):
                    ctx.lz4_encode_device([(buf.data_ptr(), nbytes)], lout.data_ptr(), lcap, res.data_ptr())
                    if step:                                   # step 0 warms up
                        enc.append((ctx.last_kernel_ms(), ctx.lz4_encode_stage_ms()))
                lres = result(api.Lz4Result)
                for step in range(args.steps + 1):
                    ctx.lz4_decode_device(lout.data_ptr(), lres["bytes_out"], back.data_ptr(), nbytes, res.data_ptr())
                    if step:
                        dec.append((ctx.last_kernel_ms(), ctx.lz4_decode_stage_ms()))
                dres = result(api.Lz4DecodeResult)
                same = bool((back == buf).all())
                for step in range(args.steps + 1):
                    ctx.deflate_indexed_device([(buf.data_ptr(), nbytes)], zout.data_ptr(), zcap, zidx.data_ptr(), entries,
                                               res.data_ptr())
                    if step:
                        zenc.append((ctx.last_kernel_ms(), ctx.deflate_stage_ms()))
                zres = result(api.DeflateResult)
                for step in range(args.steps + 1):
                    ctx.inflate_device(zout.data_ptr(), zres["bytes_out"], zidx.data_ptr(), entries, back.data_ptr(), nbytes,
                                       res.data_ptr())
                    if step:
                        zdec.append((ctx.last_kernel_ms(), ctx.inflate_stage_ms()))
                (e, es), (d, ds), (ze, zes), (zd, zds) = best_of(enc), best_of(dec), best_of(zenc), best_of(zdec)
                row = {"row": "lz4", "format": fmt.name, "payload": what, "size": n, "bytes": nbytes, "steps": args.steps,
                       "frame_bytes": lres["bytes_out"], "frame_over_raw": round(lres["bytes_out"]/nbytes, 4),
                       "zlib_stream_bytes": zres["bytes_out"], "zlib_over_raw": round(zres["bytes_out"]/nbytes, 4),
                       "result": lres, "decode_status": dres["status"], "round_trip": same,
                       "encode_ms_best": round(e[0], 4), "encode_ms_spread": es,
                       "encode_stage_ms": {k: round(v, 4) for k, v in e[1].items()},
                       "decode_ms_best": round(d[0], 4), "decode_ms_spread": ds,
                       "decode_stage_ms": {k: round(v, 4) for k, v in d[1].items()},
                       "decode_gbytes_per_s": round(nbytes/d[0]/1e6, 3),
                       "deflate_ms_best": round(ze[0], 4), "deflate_ms_spread": zes,
                       "inflate_ms_best": round(zd[0], 4), "inflate_ms_spread": zds,
                       "inflate_stage_ms": {k: round(v, 4) for k, v in zd[1].items()},
                       "encode_over_deflate": round(e[0]/ze[0], 3), "decode_over_inflate": round(d[0]/zd[0], 3)}
                if lib is not None:
                    frame = lout[:lres["bytes_out"]].cpu().numpy().tobytes()
                    host = []
                    for step in range(args.steps + 1):
                        t = time.perf_counter()
                        dctx = ctypes.c_void_p()
                        lib.LZ4F_createDecompressionContext(ctypes.byref(dctx), 100)
                        out = np.empty(nbytes, np.uint8)
                        dn, sn = ctypes.c_size_t(nbytes), ctypes.c_size_t(len(frame))
                        r = lib.LZ4F_decompress(dctx, out.ctypes.data, ctypes.byref(dn), frame, ctypes.byref(sn), None)
                        lib.LZ4F_freeDecompressionContext(dctx)
                        up = torch.from_numpy(out).to(dev)
                        torch.cuda.synchronize()
                        if step:
                            host.append((time.perf_counter() - t)*1e3)
                        assert r == 0 and dn.value == nbytes and bool((up == buf).all())
                    row.update(host_lz4f_plus_upload_ms_best=round(min(host), 3),
                               host_lz4f_plus_upload_ms_spread=round(max(host) - min(host), 3))
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
            del plain, work, back, lout, zout, zidx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ratio:
        ratio(args)
    else:
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "lz4_bench.jsonl")
        timing(args)


if __name__ == "__main__":
    main()
