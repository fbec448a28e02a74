"""numpy float64 restatement of the quality metrics of cfhip_compare.

It takes the decoded texels in the layout Context.decode returns them, so the GPU decoder (pinned to the oracle by
tests/test_gpu_decode.py) is the only thing shared with the kernels under test."""
import numpy as np

from cuttlefish_amd.api import LAYOUT_ARRAY, Layout

SNORM = (Layout.R8_SNorm, Layout.RG8_SNorm, Layout.R16_SNorm, Layout.RG16_SNorm)
TINY = 2.0 ** -24


def normalise(decoded, layout):
    """decoded texels of a layout -> (h, w, channels) float64"""
    layout = Layout(layout)
    d = np.asarray(decoded)
    if layout == Layout.RGBA16F:
        return d.astype(np.float64)
    v = d.astype(np.float64)
    if layout in (Layout.RGBA8, Layout.R8, Layout.RG8):
        return v / 255.0
    if layout in (Layout.R8_SNorm, Layout.RG8_SNorm):
        return np.maximum(v / 127.0, -1.0)
    if layout in (Layout.R16, Layout.RG16):
        return v / 2047.0
    return np.maximum(v / 1023.0, -1.0)


def reference(ref):
    """(h, w, 4) uint8 (v/255), float16 or float32 reference -> float64, as stored"""
    ref = np.asarray(ref)
    if ref.dtype == np.uint8:
        return ref.astype(np.float64) / 255.0
    return ref.astype(np.float64)


def channel_mask(layout, mask=None):
    """bit c set: channel c compared (the layout's channels AND the mask)"""
    ch = LAYOUT_ARRAY[Layout(layout)][0]
    m = 0
    for c in range(ch):
        if mask is None or mask[c]:
            m |= 1 << c
    return m


def gaussian_taps():
    """the 11 normalised taps exp(-k^2/4.5), k = -5..5, computed in double and rounded to float"""
    k = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-k * k / 4.5)
    return (w / w.sum()).astype(np.float32).astype(np.float64)


def _filter(img, w):
    """separable 11-tap filter, valid part only: (h, w) -> (h - 10, w - 10)"""
    h, wd = img.shape
    rows = sum(w[t] * img[:, t:wd - 10 + t] for t in range(11))
    return sum(w[t] * rows[t:h - 10 + t, :] for t in range(11))


def ssim_channel(x, y, data_range):
    """mean SSIM of two (h, w) float64 images over the valid window centres; NaN if a side is below 11"""
    h, wd = x.shape
    if h < 11 or wd < 11:
        return float("nan")
    w = gaussian_taps()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = _filter(x, w), _filter(y, w)
    vx = _filter(x * x, w) - mx * mx
    vy = _filter(y * y, w) - my * my
    cxy = _filter(x * y, w) - mx * my
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return float(s.mean())


def compare(decoded, layout, ref, block, mask=None, ssim=False):
    """-> dict(sse, log_sse, ref_max, ssim: 4 floats each, channels, block_errors (by, bx), windows)"""
    layout = Layout(layout)
    d = normalise(decoded, layout)
    r = reference(ref)
    h, w = r.shape[:2]
    bw, bh = block
    by, bx = -(-h // bh), -(-w // bw)
    cm = channel_mask(layout, mask)
    hdr = layout == Layout.RGBA16F
    nan = float("nan")
    out = {"sse": [0.0] * 4, "log_sse": [0.0] * 4, "ref_max": [0.0] * 4, "ssim": [nan] * 4, "channels": cm,
           "windows": 0}
    emap = np.zeros((by * bh, bx * bw))
    ssim_on = ssim and not hdr and h >= 11 and w >= 11
    if ssim_on:
        out["windows"] = (h - 10) * (w - 10)
    rng = 2.0 if layout in SNORM else 1.0
    for c in range(4):
        if not (cm >> c) & 1:
            continue
        e = d[:, :, c] - r[:, :, c]
        out["sse"][c] = float((e * e).sum())
        emap[:h, :w] += e * e
        out["ref_max"][c] = float(r[:, :, c].max())
        if hdr:
            lg = np.log2(np.maximum(d[:, :, c], TINY)) - np.log2(np.maximum(r[:, :, c], TINY))
            out["log_sse"][c] = float((lg * lg).sum())
        else:
            out["log_sse"][c] = nan
        if ssim_on:
            out["ssim"][c] = ssim_channel(d[:, :, c], r[:, :, c], rng)
    out["block_errors"] = emap.reshape(by, bh, bx, bw).sum(axis=(1, 3))
    return out
