"""numpy twin of the value table of the standard-format unpack (include/cuttlefish_hip.h, "Standard formats"):
payload of a legal (format, type) pair -> (h, w, 4) float32.  Written from the table and the field layouts of
Vulkan's packed formats, not from the kernel: plain numpy float32 division, astype and ldexp.

    UNorm   float32(v) / float32(2^n - 1)
    SNorm   max(float32(sext v) / float32(2^(n-1) - 1), -1)
    UInt / Int   float32(v)
    Float   half -> float, or the stored 32 bits
    UFloat  B10G11R11: 5-bit exponent (bias 15), 6 / 6 / 5 mantissa bits; E5B9G9R9: m * 2^(e - 24)
Channels the format does not store: 0, 0, 0, 1."""
import numpy as np

UNORM, SNORM, UINT, INT, UFLOAT, FLOAT = range(6)
F = dict(R4G4=1, R4G4B4A4=2, B4G4R4A4=3, A4R4G4B4=4, R5G6B5=5, B5G6R5=6, R5G5B5A1=7, B5G5R5A1=8,
         A1R5G5B5=9, R8=10, R8G8=11, R8G8B8=12, B8G8R8=13, R8G8B8A8=14, B8G8R8A8=15, A8B8G8R8=16,
         A2R10G10B10=17, A2B10G10R10=18, R16=19, R16G16=20, R16G16B16=21, R16G16B16A16=22, R32=23,
         R32G32=24, R32G32B32=25, R32G32B32A32=26, B10G11R11=27, E5B9G9R9=28)
NAME = {v: k for k, v in F.items()}

# packed formats: name -> (pixel bytes, [(channel, shift, bits), ...]), channel 0..3 = r, g, b, a
PACKED = {
    "R4G4": (1, [(0, 4, 4), (1, 0, 4)]),
    "R4G4B4A4": (2, [(0, 12, 4), (1, 8, 4), (2, 4, 4), (3, 0, 4)]),
    "B4G4R4A4": (2, [(2, 12, 4), (1, 8, 4), (0, 4, 4), (3, 0, 4)]),
    "A4R4G4B4": (2, [(3, 12, 4), (0, 8, 4), (1, 4, 4), (2, 0, 4)]),
    "R5G6B5": (2, [(0, 11, 5), (1, 5, 6), (2, 0, 5)]),
    "B5G6R5": (2, [(2, 11, 5), (1, 5, 6), (0, 0, 5)]),
    "R5G5B5A1": (2, [(0, 11, 5), (1, 6, 5), (2, 1, 5), (3, 0, 1)]),
    "B5G5R5A1": (2, [(2, 11, 5), (1, 6, 5), (0, 1, 5), (3, 0, 1)]),
    "A1R5G5B5": (2, [(3, 15, 1), (0, 10, 5), (1, 5, 5), (2, 0, 5)]),
    "B8G8R8": (3, [(2, 0, 8), (1, 8, 8), (0, 16, 8)]),
    "B8G8R8A8": (4, [(2, 0, 8), (1, 8, 8), (0, 16, 8), (3, 24, 8)]),
    "A8B8G8R8": (4, [(3, 0, 8), (2, 8, 8), (1, 16, 8), (0, 24, 8)]),
    "A2R10G10B10": (4, [(3, 30, 2), (0, 20, 10), (1, 10, 10), (2, 0, 10)]),
    "A2B10G10R10": (4, [(3, 30, 2), (2, 20, 10), (1, 10, 10), (0, 0, 10)]),
}
# channel arrays: name -> (bits per channel, channels)
ARRAYS = {"R8": (8, 1), "R8G8": (8, 2), "R8G8B8": (8, 3), "R8G8B8A8": (8, 4),
          "R16": (16, 1), "R16G16": (16, 2), "R16G16B16": (16, 3), "R16G16B16A16": (16, 4),
          "R32": (32, 1), "R32G32": (32, 2), "R32G32B32": (32, 3), "R32G32B32A32": (32, 4)}


def pixel_bytes(fmt):
    name = NAME[int(fmt)]
    if name in PACKED:
        return PACKED[name][0]
    if name in ARRAYS:
        return ARRAYS[name][0]//8*ARRAYS[name][1]
    return 4


def fields(fmt):
    """[(channel, shift within the pixel in bits, bits)] of every stored field (UFloat formats included)"""
    name = NAME[int(fmt)]
    if name in PACKED:
        return list(PACKED[name][1])
    if name in ARRAYS:
        bits, n = ARRAYS[name]
        return [(c, c*bits, bits) for c in range(n)]
    if name == "B10G11R11":
        return [(0, 0, 11), (1, 11, 11), (2, 22, 10)]
    return [(0, 0, 9), (1, 9, 9), (2, 18, 9)]            # E5B9G9R9, plus the shared exponent at 27


def field_value(v, bits, typ):
    """stored field v (uint64 array holding `bits` bits) -> float32, by the table"""
    v = np.asarray(v, np.uint64)
    if typ == UNORM:
        return v.astype(np.float32)/np.float32(2**bits - 1)
    signed = v.astype(np.int64) - ((v >> np.uint64(bits - 1)).astype(np.int64) << bits)
    if typ == SNORM:
        return np.maximum(signed.astype(np.float32)/np.float32(2**(bits - 1) - 1), np.float32(-1.0))
    if typ == UINT:
        return v.astype(np.float32)
    if typ == INT:
        return signed.astype(np.float32)
    if typ == FLOAT:
        if bits == 16:
            return v.astype(np.uint16).view(np.float16).astype(np.float32)
        return v.astype(np.uint32).view(np.float32)
    raise ValueError("type %d has no per-field rule" % typ)


def small_float(v, mbits):
    """unsigned 5-bit-exponent float with mbits mantissa bits -> float32"""
    v = np.asarray(v, np.uint64).astype(np.int64)
    e, m = v >> mbits, v & ((1 << mbits) - 1)
    den = np.ldexp(m.astype(np.float64), -14 - mbits)
    nor = np.ldexp(1.0 + m.astype(np.float64)/(1 << mbits), (e - 15).astype(np.int32))
    special = np.where(m == 0, np.inf, np.nan)
    return np.where(e == 0, den, np.where(e == 31, special, nor)).astype(np.float32)


def pixel_words(payload, fmt, typ):
    """the pixels of a tight payload as uint64 little-endian words (16-byte pixels: two columns lo, hi)"""
    bpp = pixel_bytes(fmt)
    b = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1, bpp).astype(np.uint64)
    lo = np.zeros(len(b), np.uint64)
    hi = np.zeros(len(b), np.uint64)
    for k in range(min(bpp, 8)):
        lo |= b[:, k] << np.uint64(8*k)
    for k in range(8, bpp):
        hi |= b[:, k] << np.uint64(8*(k - 8))
    return lo, hi


def unpack(payload, fmt, typ, width, height):
    """payload bytes of width*height pixels -> (height, width, 4) float32"""
    fmt, typ = int(fmt), int(typ)
    lo, hi = pixel_words(np.asarray(payload, np.uint8)[:width*height*pixel_bytes(fmt)], fmt, typ)
    out = np.zeros((len(lo), 4), np.float32)
    out[:, 3] = 1.0
    name = NAME[fmt]
    for c, shift, bits in fields(fmt):
        src, s = (lo, shift) if shift < 64 else (hi, shift - 64)
        v = (src >> np.uint64(s)) & np.uint64(2**bits - 1)
        if name == "B10G11R11":
            out[:, c] = small_float(v, bits - 5)
        elif name == "E5B9G9R9":
            e = ((lo >> np.uint64(27)) & np.uint64(31)).astype(np.int32)
            out[:, c] = np.ldexp(v.astype(np.float64), e - 24).astype(np.float32)
        elif bits == 32 and typ == FLOAT:
            out.view(np.uint32)[:, c] = v.astype(np.uint32)        # the bits, copied
        else:
            out[:, c] = field_value(v, bits, typ)
    return out.reshape(height, width, 4)
