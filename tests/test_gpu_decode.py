"""GPU decoding (csrc/decode.hip) against the CPU oracle decoders and, directly, against the independent
decoders the oracle is pinned to (Pillow, Mesa 23.2.1) through the committed fixtures."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
from astc_cases import block_mode as _astc_block_mode    # (N, M, weight range index, dual) or None
from cuttlefish_amd import Format, Type, api, make_params, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FOOTPRINTS = [(4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8),
              (10, 10), (12, 10), (12, 12)]

# every (format, type) pair with a decoded layout
PAIRS = ([(f, 0) for f in (29, 30, 31, 32, 36, 37, 38, 39, 40)] + [(f, t) for f in (33, 34, 41, 42) for t in (0, 1)] +
         [(35, 4), (35, 5)] + [(f, t) for f in range(43, 57) for t in (0, 4)])


def _bb(fmt):
    return 8 if fmt in (29, 30, 33, 37, 38, 39, 41) else 16


def _foot(fmt):
    return FOOTPRINTS[fmt - 43] if fmt >= 43 else (4, 4)


# ---- the oracle's answer for a payload, in the GPU's layout ---------------------------------------

def _bc6h_errors(blocks):
    """blocks for which the oracle's cfo_decode_bc6h reports a reserved mode"""
    L = O.lib()
    L.cfo_decode_bc6h.restype = ctypes.c_int
    L.cfo_decode_bc6h.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    px = np.zeros(48, np.uint16)
    b = np.ascontiguousarray(blocks.reshape(-1, 16))
    return sum(1 for i in range(b.shape[0]) if L.cfo_decode_bc6h(b[i].ctypes.data, 0, px.ctypes.data) != 0)


def oracle_decode(blocks, fmt, typ, w, h):
    """-> (array in the layout of Context.decode, error blocks)"""
    if fmt in (29, 30, 31, 32, 36):
        return O.decode(blocks, fmt, w, h), 0
    if fmt in (33, 34):
        rgba = O.decode(blocks, fmt, w, h, typ)
        ch = 1 if fmt == 33 else 2
        out = rgba[:, :, :ch].copy()
        return (out.view(np.int8) if typ == 1 else out), 0
    if fmt == 35:
        rgb = O.decode_bc6h(blocks, w, h, typ).view(np.uint16)
        out = np.full((h, w, 4), 0x3C00, np.uint16)
        out[:, :, :3] = rgb
        return out.view(np.float16), _bc6h_errors(blocks)
    if 37 <= fmt <= 40:
        return O.decode_etc(blocks, fmt, w, h), 0
    if fmt in (41, 42):
        v = O.decode_eac(blocks, fmt, w, h, typ)
        return v.astype(np.int16 if typ == 1 else np.uint16), 0
    if typ == 4:
        return O.decode_astc_hdr(blocks, fmt, w, h)
    return O.decode_astc(blocks, fmt, w, h)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    ua, ub = a.view(np.uint8), b.view(np.uint8)
    if np.array_equal(ua, ub):
        return True
    ys, xs = np.nonzero((ua != ub).any(axis=2))
    print("%d texels differ; first at (x %d, y %d): got %s, want %s" % (len(ys), xs[0], ys[0], ua[ys[0], xs[0]],
                                                                      ub[ys[0], xs[0]]))
    return False


# ---- random bitstreams ------------------------------------------------------------------------------

_WQ = [(1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 1), (1, 1, 0), (3, 0, 0), (1, 0, 1), (2, 1, 0), (4, 0, 0),
       (2, 0, 1), (3, 1, 0), (5, 0, 0)]


def _astc_legal_modes(bw, bh):
    """block modes whose grid fits the footprint and whose weights take 24..96 bits: every legal grid,
    dual-plane ones and grids the encoder never emits included"""
    out = []
    for mode in range(2048):
        if (mode & 0x1FF) == 0x1FC:
            continue
        bm = _astc_block_mode(mode)
        if bm is None:
            continue
        N, M, wq, dual = bm
        nw = N * M * (2 if dual else 1)
        bits, t, q = _WQ[wq]
        wbits = nw * bits + (8 * nw + 4) // 5 * t + (7 * nw + 2) // 3 * q
        if N <= bw and M <= bh and nw <= 64 and 24 <= wbits <= 96:
            out.append(mode)
    return np.array(out, np.uint16)


def random_payload(fmt, nblocks, seed):
    rng = np.random.default_rng(1000 + seed)
    b = rng.integers(0, 256, (nblocks, _bb(fmt)), dtype=np.uint8)
    if fmt >= 43:
        # three blocks in four get a legal block mode (all partition counts, seeds and endpoint modes stay
        # random); a slice of them becomes void extent; the rest stays fully random (mostly illegal)
        bw, bh = _foot(fmt)
        modes = _astc_legal_modes(bw, bh)
        lo = b[:, 0].astype(np.uint16) | (b[:, 1].astype(np.uint16) << 8)
        pick = rng.random(nblocks)
        legal = modes[rng.integers(0, len(modes), nblocks)]
        lo = np.where(pick < 0.75, (lo & 0xF800) | legal, lo)
        ve = pick > 0.95
        lo = np.where(ve, (lo & 0xFE00) | 0x1FC | (rng.integers(0, 2, nblocks) << 9).astype(np.uint16), lo)
        b[:, 0] = (lo & 255).astype(np.uint8)
        b[:, 1] = (lo >> 8).astype(np.uint8)
        b[ve, 1] |= 0xFC                                     # bits 10, 11: the void-extent marker
        b[ve, 2:8] = 0xFF                                    # extent all ones (legal) ...
        b[ve & (pick > 0.98), 3] = 0x00                      # ... or not
    return b.reshape(-1)


@pytest.mark.parametrize("fmt,typ", PAIRS)
def test_random_bitstreams_equal_the_oracle(gpu_ctx, fmt, typ):
    bw, bh = _foot(fmt)
    w, h = 64 * bw - (bw - 1), 64 * bh - (bh // 2 + 1)    # ragged: partial edge blocks on both sides
    blocks = random_payload(fmt, 64 * 64, fmt * 8 + typ)
    got, bad = gpu_ctx.decode(blocks, fmt, typ, w, h)
    want, want_bad = oracle_decode(blocks, fmt, typ, w, h)
    assert _same(got, want)
    assert bad == want_bad
    if fmt >= 43:
        assert 0 < bad < 4096 * 0.9          # the draw covers legal and illegal blocks
    if fmt == 35:
        assert bad > 0


# ---- independent pins ----------------------------------------------------------------------------

def test_bcn_equal_pillow(gpu_ctx):
    d = np.load(os.path.join(GOLD, "pillow_decode.npz"))
    for name, fmt in (("bc1", 29), ("bc2", 31), ("bc3", 32), ("bc7", 36)):
        blk = d[name + "_blocks"]
        n = blk.shape[0]
        got, _ = gpu_ctx.decode(blk.reshape(-1), fmt, 0, 4 * n, 4)
        got = got.reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)
        assert np.array_equal(got, d[name + "_pixels"]), name
    blk = d["bc4u_blocks"]
    n = blk.shape[0]
    got, _ = gpu_ctx.decode(blk.reshape(-1), 33, 0, 4 * n, 4)
    assert np.array_equal(got.reshape(4, n, 4).transpose(1, 0, 2).reshape(n, 16), d["bc4u_pixels"][:, :, 0])
    blk = d["bc5u_blocks"]
    got, _ = gpu_ctx.decode(blk.reshape(-1), 34, 0, 4 * n, 4)
    got = got.reshape(4, n, 4, 2).transpose(1, 0, 2, 3).reshape(n, 16, 2)
    assert np.array_equal(got, d["bc5u_pixels"][:, :, :2])


def _mesa_dims(blocks, bs):
    n = blocks.size // bs
    return 128, 4 * n // 32


@pytest.mark.parametrize("name,fmt,typ,bs", [("etc2_rgb", 38, 0, 8), ("etc2_rgba1", 39, 0, 8),
                                             ("etc2_rgba8", 40, 0, 16), ("bc7", 36, 0, 16)])
def test_etc2_bc7_equal_mesa(gpu_ctx, name, fmt, typ, bs):
    fix = np.load(os.path.join(GOLD, "mesa_blocks.npz"))
    blk = fix[name + "_blocks"]
    w, h = _mesa_dims(blk, bs)
    got, _ = gpu_ctx.decode(blk, fmt, typ, w, h)
    assert np.array_equal(got, fix[name + "_rgba"])


@pytest.mark.parametrize("name,fmt,bs", [("eac_r11", 41, 8), ("eac_rg11", 42, 16)])
@pytest.mark.parametrize("typ,tn", [(0, "u"), (1, "s")])
def test_eac_equal_mesa(gpu_ctx, name, fmt, bs, typ, tn):
    fix = np.load(os.path.join(GOLD, "mesa_blocks.npz"))
    blk = fix["%s_%s_blocks" % (name, tn)]
    w, h = _mesa_dims(blk, bs)
    got, _ = gpu_ctx.decode(blk, fmt, typ, w, h)
    v = got.astype(np.int64)
    if typ == 0:                          # Mesa returns the 16-bit replication of the 11-bit value
        e = (v << 5) | (v >> 6)
    else:
        m = np.abs(v)
        e = np.sign(v) * ((m << 5) | (m >> 5))
    assert np.array_equal(e, fix["%s_%s_px16" % (name, tn)].astype(np.int64))


@pytest.mark.parametrize("typ,tn", [(4, "uf16"), (5, "sf16")])
def test_bc6h_halves_equal_mesa(gpu_ctx, typ, tn):
    fix = np.load(os.path.join(GOLD, "mesa_blocks.npz"))
    blk = fix["bc6h_%s_blocks" % tn]
    w, h = _mesa_dims(blk, 16)
    got, _ = gpu_ctx.decode(blk, 35, typ, w, h)
    got = got.view(np.uint16)
    assert np.array_equal(got[:, :, :3], fix["bc6h_%s_half" % tn])
    assert (got[:, :, 3] == 0x3C00).all()


@pytest.mark.parametrize("fi", range(14))
def test_astc_equal_mesa(gpu_ctx, fi):
    fix = np.load(os.path.join(GOLD, "mesa_astc.npz"))
    bw, bh = FOOTPRINTS[fi]
    blk = fix["blocks_%dx%d" % (bw, bh)]
    n = blk.shape[0]
    got, _ = gpu_ctx.decode(blk.reshape(-1), 43 + fi, 0, bw * n, bh)
    got = got.reshape(bh, n, bw, 4).transpose(1, 0, 2, 3).reshape(n, bh * bw, 4)
    assert np.array_equal(got, fix["rgba_%dx%d" % (bw, bh)])


# ---- full-size round trips ------------------------------------------------------------------------

def test_full_size_bc7_and_astc_round_trip(gpu_ctx):
    img = synth.photo(4096, 4096, seed=7)
    for fmt in (Format.BC7, Format.ASTC_6x6):
        payload = gpu_ctx.encode([img], make_params(fmt, Type.UNorm, 2))[0]
        got, bad = gpu_ctx.decode(payload, fmt, Type.UNorm, 4096, 4096)
        want, want_bad = oracle_decode(payload, int(fmt), 0, 4096, 4096)
        assert np.array_equal(got, want), fmt
        assert bad == want_bad == 0
        sse = gpu_ctx.decode_sse(payload, img, fmt, Type.UNorm)
        d = want.astype(np.int64) - img.astype(np.int64)
        assert sse == [int(v) for v in (d * d).sum(axis=(0, 1))]
        assert api.psnr_from_sse(sse, 4096 * 4096) > 30.0


# ---- SSE ---------------------------------------------------------------------------------------------

def _numpy_sse(dec, ref, ch):
    d = dec[:, :, :ch].astype(np.int64) - ref[:, :, :ch].astype(np.int64)
    s = [int(v) for v in (d * d).sum(axis=(0, 1))]
    return s + [0] * (4 - ch)


SSE_PAIRS = [(29, 0), (30, 0), (31, 0), (32, 0), (33, 0), (34, 0), (36, 0), (37, 0), (38, 0), (39, 0), (40, 0),
             (43, 0), (47, 0), (50, 0), (56, 0)]


@pytest.mark.parametrize("fmt,typ", SSE_PAIRS)
def test_decode_sse_host_and_device_equal_numpy(gpu_ctx, fmt, typ):
    import torch
    bw, bh = _foot(fmt)
    w, h = 40 * bw - 3, 23 * bh - 1
    bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
    blocks = random_payload(fmt, bx * by, 77 + fmt)
    rng = np.random.default_rng(fmt)
    wide = rng.integers(0, 256, (h, w + 5, 4), dtype=np.uint8)
    ref = wide[:, :w]                                     # pitched: 4 * (w + 5) bytes between rows
    dec, _ = oracle_decode(blocks, fmt, typ, w, h)
    ch = dec.shape[2]
    want = _numpy_sse(dec, ref, ch)
    assert gpu_ctx.decode_sse(blocks, ref, fmt, typ) == want
    dev = torch.device("cuda", 0)
    d_blocks = torch.from_numpy(blocks).to(dev)
    d_ref = torch.from_numpy(np.ascontiguousarray(wide)).to(dev)
    d_sse = torch.full((4,), -1, dtype=torch.int64, device=dev)    # the call zeroes it
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu_ctx.decode_sse_device(d_blocks.data_ptr(), fmt, typ, w, h, d_ref.data_ptr(), 4 * (w + 5),
                              d_sse.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert [int(v) for v in d_sse.cpu()] == want


# ---- device path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,typ", [(29, 0), (33, 1), (34, 0), (35, 5), (36, 0), (40, 0), (42, 1), (44, 0),
                                     (55, 4)])
def test_device_path_on_a_torch_stream_equals_host(gpu_ctx, fmt, typ):
    import torch
    bw, bh = _foot(fmt)
    w, h = 33 * bw - 1, 17 * bh - 2
    bx, by = (w + bw - 1) // bw, (h + bh - 1) // bh
    blocks = random_payload(fmt, bx * by, 500 + fmt)
    want, want_bad = gpu_ctx.decode(blocks, fmt, typ, w, h)
    _, tb = api.decoded_layout(fmt, typ)
    dev = torch.device("cuda", 0)
    for pitch, offset in ((w * tb + 64, 0), (w * tb + 3, 1)):     # aligned rows, then an unaligned output
        d_blocks = torch.from_numpy(blocks).to(dev)
        d_out = torch.full((h * pitch + offset,), 0xAB, dtype=torch.uint8, device=dev)
        d_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        gpu_ctx.decode_device(d_blocks.data_ptr(), fmt, typ, w, h, d_out.data_ptr() + offset, pitch,
                              error_blocks=d_bad.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        out = d_out.cpu().numpy()[offset:].reshape(h, pitch)
        assert np.array_equal(out[:, :w * tb], want.view(np.uint8).reshape(h, w * tb))
        assert (out[:, w * tb:] == 0xAB).all()              # nothing outside the surface is written
        assert int(d_bad.cpu()[0]) == want_bad


# ---- argument errors -------------------------------------------------------------------------------

def test_argument_errors_and_a_following_encode(gpu_ctx):
    import torch
    L, h_ = gpu_ctx._lib, gpu_ctx._h
    blk = np.zeros(16 * 16, np.uint8)
    out = np.zeros(16 * 16 * 8, np.uint8)
    sse = (ctypes.c_uint64 * 4)()
    ref = np.zeros((16, 16, 4), np.uint8)

    def dec(fmt, typ, nbytes=blk.nbytes, w=16, h=16, cap=out.nbytes, bp=blk.ctypes.data, op=out.ctypes.data):
        return L.cfhip_decode(h_, fmt, typ, bp, nbytes, w, h, op, cap, None)

    assert dec(36, 0) == 0
    assert dec(14, 0) == api.E_UNSUPPORTED                  # a standard format
    assert dec(36, 1) == api.E_UNSUPPORTED                  # BC7 SNorm
    assert dec(35, 0) == api.E_UNSUPPORTED                  # BC6H UNorm
    assert dec(36, 0, w=0) == api.E_INVALID
    assert dec(36, 0, bp=None) == api.E_INVALID
    assert dec(36, 0, op=None) == api.E_INVALID
    assert dec(36, 0, nbytes=blk.nbytes - 1) == api.E_INVALID
    assert dec(36, 0, cap=16 * 16 * 4 - 1) == api.E_CAPACITY
    assert b"out_capacity" in L.cfhip_last_error(h_)
    assert dec(35, 4, cap=16 * 16 * 8 - 1) == api.E_CAPACITY
    assert L.cfhip_decode_sse(h_, 35, 4, blk.ctypes.data, blk.nbytes, 16, 16, ref.ctypes.data, 64, sse) == \
        api.E_UNSUPPORTED
    assert L.cfhip_decode_sse(h_, 41, 0, blk.ctypes.data, blk.nbytes, 16, 16, ref.ctypes.data, 64, sse) == \
        api.E_UNSUPPORTED
    assert L.cfhip_decode_sse(h_, 33, 1, blk.ctypes.data, blk.nbytes, 16, 16, ref.ctypes.data, 64, sse) == \
        api.E_UNSUPPORTED
    assert L.cfhip_decode_sse(h_, 36, 0, blk.ctypes.data, blk.nbytes, 16, 16, ref.ctypes.data, 63, sse) == \
        api.E_INVALID
    assert L.cfhip_decode_sse(h_, 36, 0, blk.ctypes.data, blk.nbytes, 16, 16, None, 64, sse) == api.E_INVALID
    assert L.cfhip_decode_sse(h_, 36, 0, blk.ctypes.data, blk.nbytes, 16, 16, ref.ctypes.data, 64, None) == \
        api.E_INVALID

    # a rejected device decode on stream A enqueues nothing; an encode on stream B is undisturbed
    dev = torch.device("cuda", 0)
    img = synth.photo(256, 192, seed=3)
    p = make_params(Format.BC7, Type.UNorm, 2)
    want = gpu_ctx.encode([img], p)[0]
    d_blk = torch.zeros(4096, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(256 * 192 * 4, dtype=torch.uint8, device=dev)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    assert L.cfhip_decode_device(h_, 36, 0, ctypes.c_void_p(d_blk.data_ptr()), 64, 64,
                                 ctypes.c_void_p(d_out.data_ptr()), 255, None, ctypes.c_void_p(a.cuda_stream)) == \
        api.E_INVALID                                       # pitch < width * 4
    assert L.cfhip_decode_device(h_, 10, 0, ctypes.c_void_p(d_blk.data_ptr()), 64, 64,
                                 ctypes.c_void_p(d_out.data_ptr()), 256, None, ctypes.c_void_p(a.cuda_stream)) == \
        api.E_UNSUPPORTED
    assert L.cfhip_decode_sse_device(h_, 36, 0, ctypes.c_void_p(d_blk.data_ptr()), 64, 64, None, 256,
                                     ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(a.cuda_stream)) == \
        api.E_INVALID
    d_img = torch.from_numpy(img).to(dev)
    d_pay = torch.zeros(want.size, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.encode_device([dict(pixels=d_img.data_ptr(), pixel_type=0, width=256, height=192, row_pitch_bytes=1024,
                                out=d_pay.data_ptr(), out_capacity=want.size)], p, stream=b.cuda_stream)
    b.synchronize()
    assert np.array_equal(d_pay.cpu().numpy(), want)
    # and the host decode of that payload still works after the rejected calls
    got, bad = gpu_ctx.decode(want, Format.BC7, Type.UNorm, 256, 192)
    assert np.array_equal(got, O.decode(want, 36, 256, 192)) and bad == 0
