#!/usr/bin/env python3
"""Size of the zlib encoder's streams (tests/deflate_ref.py) against zlib, on the CPU.

Rows: the 32 payloads of tools/lzsize_quality.py (tests/lzsize_cases.py): oracle payloads at Quality.Normal of two
inputs 1024 x 128 for ten formats, and the BC1 / BC7 ones after rdo_ref.rdo at three lambdas each.  Per row: raw bytes,
zlib level 9 and level 1 bytes, the estimate (lzsize_ref), the twin's stream, stream / zlib-9, stream / zlib-1, the
price of integer code lengths and headers (stream - estimate) / zlib-9, and the groups per form.
Prints markdown; --out writes it.

    python tools/deflate_quality.py [--out profiles/deflate_ratio.md]
"""
import argparse
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deflate_ref as D  # noqa: E402
import lzsize_cases as C  # noqa: E402
import lzsize_ref as Z  # noqa: E402


def rows():
    """[(name, raw bytes, zlib-9, zlib-1, estimate, stream, result)]"""
    out = []
    for name, p in C.payload_rows():
        raw = p.tobytes()
        stream, res = D.deflate(p)
        assert zlib.decompress(stream) == raw, name
        out.append((name, len(raw), len(zlib.compress(raw, 9)), len(zlib.compress(raw, 1)), Z.lz_size(p)["est_bytes"],
                    len(stream), res))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# The zlib encoder's streams against zlib (CPU twin)", "",
             "`tools/deflate_quality.py`.  The 32 payload rows of `profiles/lzsize_accuracy.md`.  stream: the bytes of",
             "`tests/deflate_ref.py`, which the GPU writes exactly; estimate: `lzsize_ref`'s est_bytes for the same",
             "tokens.  (stream - estimate) / zlib-9 is what integer code lengths, the code-table headers, the closing",
             "blocks and the 6-byte wrapper cost; the test's band is the estimator's 0.95 ... 1.08 moved by its range.", "",
             "| payload | bytes | zlib-9 | zlib-1 | estimate | stream | stream / zlib-9 | stream / zlib-1 | "
             "(stream - est) / zlib-9 | stored, fixed, dynamic |", "|---|---|---|---|---|---|---|---|---|---|"]
    r9, add = [], []
    for name, n, z9, z1, est, size, res in rows():
        r9.append(size/z9)
        add.append((size - est)/z9)
        lines.append("| %s | %d | %d | %d | %d | %d | %.4f | %.4f | %.4f | %d, %d, %d |" % (
            name, n, z9, z1, est, size, size/z9, size/z1, (size - est)/z9, res["blocks_stored"], res["blocks_fixed"],
            res["blocks_dynamic"]))
    lines += ["", "stream / zlib-9: %.4f ... %.4f" % (min(r9), max(r9)),
              "", "(stream - estimate) / zlib-9: %.4f ... %.4f" % (min(add), max(add))]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
