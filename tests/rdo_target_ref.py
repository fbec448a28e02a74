"""The rate-distortion pass to a target ratio in numpy -- THE DEFINITION of what cfhip_rdo_target computes (DESIGN.md
section 4.15): rdo_ref / rdo2d_ref and lzsize_ref composed as the library composes its kernels.

The stream is the surfaces' payloads concatenated in call order.  T = floor(ratio est(plain)); hi = round(16 lambda);
the pass at hi from the pristine payloads; estimate > T: that pass, reached = 0.  Otherwise lo = 0 and, while
hi - lo > 1: mid = (lo + hi) // 2, hi = mid if est(mid) <= T else lo = mid; the pass at hi, reached = 1.  trials counts
the passes estimated."""
import math

import numpy as np

import lzsize_ref
import rdo2d_ref
import rdo_ref


def pass_at(payloads, sources, fmt, typ, lam16, max_sse_increase=None, mask=(True,)*4, row_above=False,
            window_bytes=rdo2d_ref.WINDOW):
    """the pass at lambda = lam16 / 16 over every surface -> (payloads, statistics)"""
    lam = lam16/16.0
    res = []
    for p, s in zip(payloads, sources):
        if row_above:
            res.append(rdo2d_ref.rdo2d(p, s, fmt, typ, lam, max_sse_increase, mask, True, window_bytes))
        else:
            res.append(_rdo_lam16(p, s, fmt, typ, lam16, max_sse_increase, mask))
    return [r[0] for r in res], [r[1] for r in res]


def _rdo_lam16(p, s, fmt, typ, lam16, cap, mask):
    if lam16 == 0:
        raise ValueError("the search never runs the pass at 0")
    return rdo_ref.rdo(p, s, fmt, typ, lam16/16.0, cap, mask)


def rdo_target(payloads, sources, fmt, typ=rdo_ref.UNORM, target_ratio=0.85, lam=32.0, max_sse_increase=None,
               mask=(True,)*4, row_above=False, window_bytes=rdo2d_ref.WINDOW, estimate=None):
    """-> (payloads, statistics, result dict).  estimate: the size function of a list of payloads (None: the twin's
    est_bytes); measurements pass zlib here."""
    ratio = float(np.float32(target_ratio))
    if not (0.0 < ratio < 1.0):
        raise ValueError("target_ratio outside (0, 1)")
    if estimate is None:
        estimate = lambda parts: lzsize_ref.lz_size(parts)["est_bytes"]          # noqa: E731
    plain = [np.asarray(p, np.uint8).reshape(-1) for p in payloads]
    est_plain = estimate(plain)
    target = int(math.floor(ratio*float(est_plain)))
    seen = {}

    def trial(lam16):
        outs, stats = pass_at(plain, sources, fmt, typ, lam16, max_sse_increase, mask, row_above, window_bytes)
        seen[lam16] = (outs, stats, estimate(outs))
        return seen[lam16][2]

    hi, lo = rdo_ref.lambda16(lam), 0
    reached = trial(hi) <= target
    while reached and hi - lo > 1:
        mid = (lo + hi)//2
        if trial(mid) <= target:
            hi = mid
        else:
            lo = mid
    outs, stats, est = seen[hi]
    return outs, stats, dict(lambda16=hi, reached=int(reached), trials=len(seen), est_bytes_plain=int(est_plain),
                             est_bytes_final=int(est))
