"""THE DEFINITION of the PNG files cfhip_png_encode writes (csrc/png.hip): numpy for the samples
and the filters, tests/deflate_ref.py for the zlib stream, zlib.crc32 for the CRCs.

One file: the signature, IHDR (depth 8 or 16; colour type 0, 2, 4 or 6; no interlace), an sRGB chunk with rendering
intent 0 for an sRGB image, exactly one IDAT chunk holding one zlib stream, IEND.

Samples.  The source is an (h, w, 4) image of uint8, float16 or float32.  Floats: round(clamp(f, 0, 1) x 255) or x 65535,
the product taken in float32 and rounded through floor(x + 0.5) in double, NaN -> 0.  uint8 at depth 16: v x 257.  Grey
takes the red channel, colour types without alpha drop it, 16-bit samples are big-endian.

Filtering.  Every row gets the type, 0 to 4, with the smallest sum over its filtered bytes of (b < 128 ? b : 256 - b);
the lowest type wins a tie.  Filters read the raw row above; the first row sees zeros; a and c lie bpp bytes back.
"""
import struct
import zlib

import numpy as np

import deflate_ref

SIGNATURE = b"\x89PNG\r\n\x1a\n"
GREY, RGB, GREY_ALPHA, RGBA = 0, 2, 4, 6
COLOR_TYPES = (GREY, RGB, GREY_ALPHA, RGBA)
CHANNELS = {GREY: (0,), RGB: (0, 1, 2), GREY_ALPHA: (0, 3), RGBA: (0, 1, 2, 3)}
DEPTHS = (8, 16)
FILTERS = ("none", "sub", "up", "average", "paeth")
FIELDS = ("bytes_out", "idat_bytes", "filtered_bytes", "rows_by_filter", "idat_crc32", "deflate")


def bpp(color_type: int, bit_depth: int) -> int:
    return len(CHANNELS[color_type])*bit_depth//8


def png_bound(width: int, height: int, color_type: int, bit_depth: int, srgb: bool) -> int:
    n = height*(1 + width*bpp(color_type, bit_depth))
    return 8 + 25 + (13 if srgb else 0) + 12 + deflate_ref.deflate_bound(n) + 12


def quantise(pixels, bit_depth: int) -> np.ndarray:
    """(h, w, 4) uint8 / float16 / float32 -> the samples, int64"""
    a = np.asarray(pixels)
    top = 255 if bit_depth == 8 else 65535
    if a.dtype == np.uint8:
        return a.astype(np.int64)*(1 if bit_depth == 8 else 257)
    assert a.dtype in (np.float16, np.float32), a.dtype
    f = a.astype(np.float32)
    with np.errstate(invalid="ignore"):
        f = np.where(f > 0, np.where(f < 1, f, np.float32(1)), np.float32(0)).astype(np.float32)   # NaN > 0 is false
    p = (f*np.float32(top)).astype(np.float32)
    return np.floor(p.astype(np.float64) + 0.5).astype(np.int64)


def raw_rows(pixels, color_type: int, bit_depth: int) -> np.ndarray:
    """-> (h, w x bpp) uint8: the rows before filtering"""
    q = quantise(pixels, bit_depth)[..., list(CHANNELS[color_type])]
    h, w = q.shape[:2]
    if bit_depth == 16:
        q = np.stack([q >> 8, q & 255], axis=-1)
    return q.reshape(h, w*bpp(color_type, bit_depth)).astype(np.uint8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw: np.ndarray, pixel_bytes: int):
    """-> ((h, 1 + row bytes) uint8 the filtered rows behind their type bytes, (h,) the types)"""
    x = raw.astype(np.int64)
    h, rb = x.shape
    b = np.vstack([np.zeros((1, rb), np.int64), x[:-1]])
    a = np.hstack([np.zeros((h, pixel_bytes), np.int64), x[:, :-pixel_bytes]])[:, :rb]
    c = np.hstack([np.zeros((h, pixel_bytes), np.int64), b[:, :-pixel_bytes]])[:, :rb]
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth(a, b, c)]) & 255      # (5, h, rb)
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                            # (5, h)
    types = np.argmin(cost, axis=0)                                                      # the first of the smallest
    out = np.empty((h, 1 + rb), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return out, types


def filtered(pixels, color_type: int, bit_depth: int):
    """-> (the zlib stream's input as bytes, rows per filter type)"""
    rows, types = filter_rows(raw_rows(pixels, color_type, bit_depth), bpp(color_type, bit_depth))
    return rows.tobytes(), [int((types == t).sum()) for t in range(5)]


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def assemble(width, height, color_type, bit_depth, srgb, idat: bytes) -> bytes:
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bit_depth, color_type, 0, 0, 0))
    if srgb:
        out += chunk(b"sRGB", b"\x00")
    return out + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def encode(pixels, color_type: int = RGBA, bit_depth: int = 8, srgb: bool = False):
    """-> (the file, the fields of cfhip_png_result)"""
    a = np.asarray(pixels)
    h, w = a.shape[:2]
    assert h and w and color_type in COLOR_TYPES and bit_depth in DEPTHS
    data, rows = filtered(a, color_type, bit_depth)
    assert len(data) < 1 << 31
    z, dres = deflate_ref.deflate(np.frombuffer(data, np.uint8))
    out = assemble(w, h, color_type, bit_depth, srgb, z)
    assert len(out) <= png_bound(w, h, color_type, bit_depth, srgb)
    return out, {"bytes_out": len(out), "idat_bytes": len(z), "filtered_bytes": len(data), "rows_by_filter": rows,
                 "idat_crc32": zlib.crc32(b"IDAT" + z), "deflate": dres}


def twin(pixels, color_type: int = RGBA, bit_depth: int = 8, srgb: bool = False) -> bytes:
    return encode(pixels, color_type, bit_depth, srgb)[0]


# ---- the images the tests share --------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 7), (7, 1), (5, 3), (67, 29))             # (width, height)
DTYPES = (np.uint8, np.float16, np.float32)


def image(width: int, height: int, dtype, seed: int = 0) -> np.ndarray:
    """Smooth gradients with noise and a few specials: rows that favour different filters, values outside [0, 1]"""
    rng = np.random.default_rng(seed*1000003 + width*131 + height)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    base = np.stack([(x*3 + y*5) % 97/96.0, (x*x + y) % 53/52.0, np.sin(x/5.0 + y/3.0)*0.6 + 0.5,
                     (x + 2*y) % 11/10.0], axis=-1)
    f = base + rng.normal(0, 0.02, base.shape)
    f[rng.random(base.shape) < 0.02] = 1.5
    f[rng.random(base.shape) < 0.02] = -0.25
    if dtype == np.uint8:
        return np.clip(np.round(f*255), 0, 255).astype(np.uint8)
    return f.astype(dtype)


def five_filter_image() -> np.ndarray:
    """(10, 64, 4) uint8 whose red channel, as grey at depth 8 (rows of 64 bytes, bpp 1), makes every filter win a row:
    five pairs of (the row above, the row)."""
    x = np.arange(64)
    noisy = (37*x + 11) % 251
    avg = np.zeros(64, np.int64)
    for i in range(64):
        avg[i] = ((avg[i - 1] if i else 0) + noisy[i]) >> 1
    rows = [x % 2 ^ 1, x % 2,                                   # alternating 1/0 above alternating 0/1 -> None
            noisy, (3*x) % 256,                                 # -> Sub
            noisy, noisy,                                       # -> Up
            noisy, avg,                                         # -> Average (sum 0)
            np.where(x < 20, 10, 200) + x % 3, np.where(x < 32, 10, 200) + x % 3]     # -> Paeth
    img = np.zeros((10, 64, 4), np.uint8)
    img[..., 0] = np.array(rows, np.int64)
    img[..., 3] = 255
    return img


# ---- a reader written from the specification (not from the filter code above) ------------------------------------------
def read_chunks(data: bytes):
    """-> [(type, data)], every CRC checked"""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def read(data: bytes):
    """-> ((h, w, channels) samples, depth, colour type, whether an sRGB chunk is there, the filter types)"""
    chunks = read_chunks(data)
    kinds = [k for k, _ in chunks]
    assert kinds in ([b"IHDR", b"IDAT", b"IEND"], [b"IHDR", b"sRGB", b"IDAT", b"IEND"]), kinds
    w, h, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, flt, lace) == (0, 0, 0) and depth in DEPTHS and ct in COLOR_TYPES
    srgb = kinds[1] == b"sRGB"
    if srgb:
        assert chunks[1][1] == b"\x00"
    step = len(CHANNELS[ct])*depth//8
    line = w*step
    raw = zlib.decompress(chunks[-2][1])
    assert len(raw) == h*(1 + line)
    rows, types = [], []
    prev = bytearray(line)
    for y in range(h):
        t = raw[y*(1 + line)]
        cur = bytearray(raw[y*(1 + line) + 1:(y + 1)*(1 + line)])
        for i in range(line):
            left = cur[i - step] if i >= step else 0
            above = prev[i]
            corner = prev[i - step] if i >= step else 0
            if t == 1:
                pred = left
            elif t == 2:
                pred = above
            elif t == 3:
                pred = (left + above)//2
            elif t == 4:
                p = left + above - corner
                da, db, dc = abs(p - left), abs(p - above), abs(p - corner)
                pred = left if da <= db and da <= dc else above if db <= dc else corner
            else:
                assert t == 0
                pred = 0
            cur[i] = (cur[i] + pred) & 255
        rows.append(bytes(cur))
        types.append(t)
        prev = cur
    a = np.frombuffer(b"".join(rows), np.uint8).reshape(h, w, len(CHANNELS[ct]), depth//8).astype(np.int64)
    samples = a[..., 0] if depth == 8 else (a[..., 0] << 8) | a[..., 1]
    return samples, depth, ct, srgb, types
