"""PVRTC1 4 bpp on the MI355X at the sizes and inputs where a kernel can be wrong unseen.  No outside PVRTC decoder
exists on the build machines, so these stand in for one: (A) the encoder byte for byte at full size, through
surfaces that repeat a tile (the twin encodes the tile only; tests/test_pvrtc_ref.py proves the symmetry on the
twin), one non-periodic surface against the twin directly, and a repeated call; (B) the decoder and its fused SSE
above 2^20 texels and on long grids; (C) many surfaces in one call, the cube with its mip tail, and the device
entry with pitches, float sources and unaligned outputs; (D) float specials and zero-weight masks; (E) one
hand-derived vector per colour field; (F) the alignment check of the device SSE entries.  Every comparison is exact."""
import numpy as np
import pytest

import pvrtc_ref as P
from cuttlefish_amd import Format, Quality, Texture, Type, api, make_params, synth
from cuttlefish_amd.texture import CubeFace, Dimension
from test_pvrtc_ref import (FIELD_VECTORS, TWO_COLOUR_VECTORS, check_constant_vector, first_block_difference, retile,
                            special_source, tile_content)

pytestmark = pytest.mark.gpu

RGB, RGBA = Format.PVRTC1_RGB_4BPP, Format.PVRTC1_RGBA_4BPP
CANARY = 0xA5

_twin_cache = {}


def twin_tile(tw, th, kind, fmt, q):
    """the tile and the twin's payload of it alone (each computed once per session)"""
    key = (tw, th, kind, int(fmt), int(q))
    tile = tile_content(tw, th, kind, seed=tw + 3 * th)
    if key not in _twin_cache:
        _twin_cache[key] = P.encode(tile, int(fmt), int(q))
    return tile, _twin_cache[key]


# ---- A. the encoder byte for byte at full size ----------------------------------------------------------------
# (surface w, h, tile w, h, alpha content, source type, levels)
TILED = [
    (2048, 2048, 64, 64, "graded", "u8", list(Quality)),
    (4096, 1024, 32, 64, "cutout", "f32", [Quality.Normal, Quality.Highest]),
    (512, 8192, 64, 16, "graded", "u8", [Quality.Normal, Quality.Highest]),
    (4096, 4096, 64, 64, "cutout", "u8", [Quality.Normal, Quality.Highest]),
]


@pytest.mark.parametrize("fmt", [RGB, RGBA])
@pytest.mark.parametrize("w, h, tw, th, kind, typ, levels", TILED, ids=["%dx%d" % c[:2] for c in TILED])
def test_tiled_surface_matches_twin_of_tile(gpu_ctx, fmt, w, h, tw, th, kind, typ, levels):
    """A surface that repeats a tile is, on the torus PVRTC1 lives on, the tile seen at every shift by an even
    number of blocks: its payload must be the twin's blocks of the tile, re-indexed.  Up to 2^20 refine wavefronts
    per phase run here under a byte comparison."""
    for q in levels:
        tile, small = twin_tile(tw, th, kind, fmt, q)
        big = np.tile(tile, (h // th, w // tw, 1))
        if typ == "f32":
            big = big.astype(np.float32) / np.float32(255)
            assert np.array_equal(P.to_rgba8(big[:th, :tw]), tile)
        got = gpu_ctx.encode_pvrtc([big], make_params(fmt, Type.UNorm, q))[0]
        diff = first_block_difference(got, retile(small, tw, th, w, h), tw, th, w, h)
        assert diff is None, (q, diff)


@pytest.mark.parametrize("fmt", [RGB, RGBA])
def test_non_periodic_surface_matches_twin(gpu_ctx, fmt):
    """Tiling cannot see a wrong wrap at the surface's edge (it looks like a correct continuation), so one surface
    without any period goes through the twin whole.  The twin's Normal encode of the RGBA format, one CPU core:
    1024 x 1024 18 s, 2048 x 1024 34 s, 2048 x 2048 70 s (1.8 GiB); 2048 x 2048 is the largest power-of-two size
    at about a minute (the GPU host's cores run it in 22 to 26 s).  Left and right, top and bottom edges differ in
    colour and alpha."""
    n = 2048
    img = synth.photo(n, n, seed=21)
    yy, xx = np.mgrid[0:n, 0:n]
    img[..., 3] = np.clip(255 - (xx + 2 * yy) // 24, 0, 255)
    img[..., 0] = np.clip(img[..., 0].astype(np.int64) // 2 + xx // 16, 0, 255)
    got = gpu_ctx.encode_pvrtc([img], make_params(fmt, Type.UNorm, Quality.Normal))[0]
    diff = first_block_difference(got, P.encode(img, int(fmt), 2), n, n, n, n)
    assert diff is None, diff


def test_same_call_twice_gives_the_same_bytes(gpu_ctx):
    """a race between the wavefronts of a refine phase shows as a difference between two runs of one call"""
    img = synth.photo(4096, 4096, seed=5)
    img[..., 3] = (img[..., 1].astype(np.int64) * 3 + img[..., 0]) % 256
    p = make_params(RGBA, Type.UNorm, Quality.Highest)
    a = gpu_ctx.encode_pvrtc([img], p)[0]
    b = gpu_ctx.encode_pvrtc([img], p)[0]
    diff = first_block_difference(b, a, 4096, 4096, 4096, 4096)
    assert diff is None, diff


# ---- B. the decoder and the fused SSE above 2^20 texels and on long grids ---------------------------------------
def exact_sse(dec, ref):
    d = dec.astype(np.int32) - ref.astype(np.int32)
    return [int(v) for v in (d * d).sum(axis=(0, 1), dtype=np.int64)]


def check_decode_entries(ctx, w, h, seed):
    """random payload (all 64 bits of every block: both modes, every opacity pair), both formats: host and device
    decode against the twin, host and device SSE against the exact integer sums; the device forms with pitched
    buffers, a canary around the texels and the sums pre-filled with -1"""
    import torch
    rng = np.random.default_rng(seed)
    payload = rng.integers(0, 256, P.payload_size(w, h), dtype=np.uint8)
    ref = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pitch = 4 * w + 64
    blk = torch.from_numpy(payload).to("cuda")
    ref_p = np.full((h, pitch), CANARY, np.uint8)
    ref_p[:, :4 * w] = ref.reshape(h, 4 * w)
    ref_d = torch.from_numpy(ref_p).to("cuda")
    assert blk.data_ptr() % 8 == 0 and ref_d.data_ptr() % 4 == 0
    for fmt in (RGB, RGBA):
        want = P.decode(payload, w, h, int(fmt))
        got = ctx.decode_pvrtc(payload, fmt, w, h)
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, (fmt, "texel (x, y)", bad[0][::-1].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        sums = exact_sse(want, ref)
        assert ctx.decode_pvrtc_sse(payload, ref, fmt) == sums
        out = torch.full((h + 2, pitch), CANARY, dtype=torch.uint8, device="cuda")
        sse = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()          # the context's stream is not torch's: its fills must have landed
        ctx.decode_pvrtc_device(blk.data_ptr(), fmt, w, h, out.data_ptr() + pitch, pitch)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[1:h + 1, :4 * w].reshape(h, w, 4), want)
        assert (o[0] == CANARY).all() and (o[h + 1] == CANARY).all() and (o[:, 4 * w:] == CANARY).all()
        ctx.decode_pvrtc_sse_device(blk.data_ptr(), fmt, w, h, ref_d.data_ptr(), pitch, sse.data_ptr())
        torch.cuda.synchronize()
        assert [int(v) for v in sse.cpu()] == sums


@pytest.mark.parametrize("w, h", [(2048, 1024), (1024, 4096), (4096, 4096)])
def test_decode_and_sse_above_2_20_texels(gpu_ctx, w, h):
    """2, 4 and 16 trips of the SSE kernel's stride loop (its grid stops at 4 096 workgroups of 256 texels).  The
    twin decodes 4096 x 4096 in about 12 s per format, so every size is compared with the twin texel by texel"""
    check_decode_entries(gpu_ctx, w, h, seed=w + h)


@pytest.mark.parametrize("w, h", [(8, 4096), (4096, 8), (4, 2048), (2048, 2), (1, 1024), (32768, 8), (8, 32768)])
def test_decode_and_sse_on_long_grids(gpu_ctx, w, h):
    """the Morton index with many high bits of one side left over, up to the entries' limit of 32 768"""
    check_decode_entries(gpu_ctx, w, h, seed=w * 7 + h)


# ---- C. many surfaces in one call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, quality", [(RGBA, Quality.Low), (RGB, Quality.High)])
def test_cube_with_mips_every_payload(fmt, quality):
    """6 faces x 7 levels (64 ... 1) in one call: 42 surfaces, the 4 x 4, 2 x 2 and 1 x 1 tail repeating itself"""
    t = Texture(Dimension.Cube, 64, 64, mip_levels=Texture.allMipLevels)
    src = {}
    for face in range(6):
        for mip in range(t.mip_level_count()):
            s = 64 >> mip
            img = synth.photo(max(s, 8), max(s, 8), seed=face * 10 + mip)[:s, :s].astype(np.float32) / 255
            img[..., 3] = np.float32(((face + mip) % 3) / 2)
            assert t.set_image(img, CubeFace(face), mip)
            src[face, mip] = np.array(t.get_image(CubeFace(face), mip))
    assert t.convert(fmt, Type.UNorm, quality)
    for (face, mip), img in src.items():
        want = P.encode(img, int(fmt), int(quality))
        assert np.array_equal(t.data(CubeFace(face), mip), want), (face, mip)


BATCH_SIZES = [(1, 1), (2, 2), (4, 4), (1, 8), (8, 8), (16, 4), (4, 16), (16, 16), (32, 8), (8, 32), (2, 64),
               (32, 32), (64, 32)]


def batch_surfaces(count, seed):
    """`count` small surfaces: the sizes in turn, then shuffled; alpha content and source type vary"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        w, h = BATCH_SIZES[i % len(BATCH_SIZES)]
        img = synth.photo(max(w, 8), max(h, 8), seed=seed + i)[:h, :w].copy()
        if i % 3 == 1:
            img[..., 3] = rng.integers(0, 256, (h, w))
        elif i % 3 == 2:
            img[..., 3] = np.where(rng.integers(0, 4, (h, w)) == 0, 0, 255)
        if i % 5 == 3:
            img = img.astype(np.float32) / np.float32(255)
        elif i % 5 == 4:
            img = (img.astype(np.float32) / np.float32(255)).astype(np.float16)
        out.append(img)
    order = rng.permutation(count)
    return [out[i] for i in order]


@pytest.mark.parametrize("count", [1, 2, 3, 37, 260])
def test_batch_of_small_surfaces_every_payload(gpu_ctx, count):
    """the surface table's binary search with 1, 2, 3, a non-power-of-two count and a few hundred entries (each
    of the 13 sizes 20 times at 260); every payload against the twin"""
    imgs = batch_surfaces(count, seed=count)
    for fmt in (RGB, RGBA):
        got = gpu_ctx.encode_pvrtc(imgs, make_params(fmt, Type.UNorm, Quality.Normal))
        assert len(got) == count
        for i, (img, g) in enumerate(zip(imgs, got)):
            assert np.array_equal(g, P.encode(img, int(fmt), 2)), (i, img.shape, img.dtype)


def test_device_entry_pitches_float_sources_and_unaligned_out(gpu_ctx):
    """one encode_pvrtc_device call: a padded pitch, a negative pitch (pointer at the last row), an RGBA16F and an
    RGBA32F source; `out` 0, 4 and 1 bytes past an 8-byte boundary inside a canary-filled buffer (the header sets
    no alignment rule for it: pack's 8-byte store and, twice, its byte stores).  Payloads equal the host entry's."""
    import torch
    u8a = tile_content(32, 16, "graded", 1)
    u8b = tile_content(64, 32, "cutout", 2)
    f16 = (tile_content(16, 16, "graded", 3).astype(np.float32) / np.float32(255)).astype(np.float16)
    f32 = tile_content(8, 64, "cutout", 4).astype(np.float32) / np.float32(255)
    p = make_params(RGBA, Type.UNorm, Quality.High)
    host = gpu_ctx.encode_pvrtc([u8a, u8b, f16, f32], p)
    for img, hp in zip((u8a, u8b, f16, f32), host):
        assert np.array_equal(hp, P.encode(img, int(RGBA), 3))

    def padded(img, pad):
        h, w = img.shape[:2]
        row = w * 4 * img.itemsize
        buf = np.full((h, row + pad), CANARY, np.uint8)
        buf[:, :row] = img.reshape(h, -1).view(np.uint8)
        return torch.from_numpy(buf).to("cuda"), row + pad

    srcs = []
    d, pitch = padded(u8a, 32)
    srcs.append((d, d.data_ptr(), pitch, api.PixelType.RGBA8, u8a))
    d, pitch = padded(np.ascontiguousarray(u8b[::-1]), 16)      # stored bottom-up: the last row in memory is row 0
    srcs.append((d, d.data_ptr() + (u8b.shape[0] - 1) * pitch, -pitch, api.PixelType.RGBA8, u8b))
    d, pitch = padded(f16, 0)
    srcs.append((d, d.data_ptr(), pitch, api.PixelType.RGBA16F, f16))
    d, pitch = padded(f32, 48)
    srcs.append((d, d.data_ptr(), pitch, api.PixelType.RGBA32F, f32))
    outs, surf = [], []
    for (d, ptr, pitch, pt, img), hp, off in zip(srcs, host, (0, 4, 1, 1)):
        o = torch.full((hp.size + 32,), CANARY, dtype=torch.uint8, device="cuda")
        assert o.data_ptr() % 8 == 0
        outs.append((o, 8 + off))
        surf.append({"pixels": ptr, "pixel_type": pt, "width": img.shape[1], "height": img.shape[0],
                     "row_pitch_bytes": pitch, "out": o.data_ptr() + 8 + off, "out_capacity": hp.size})
    torch.cuda.synchronize()              # the context's stream is not torch's: the canary fills must have landed
    gpu_ctx.encode_pvrtc_device(surf, p)
    torch.cuda.synchronize()
    for i, ((o, off), hp) in enumerate(zip(outs, host)):
        o = o.cpu().numpy()
        assert np.array_equal(o[off:off + hp.size], hp), i
        assert (o[:off] == CANARY).all() and (o[off + hp.size:] == CANARY).all(), i


# ---- D. float specials and zero-weight masks ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_float_specials_through_the_load_pass(gpu_ctx, dtype):
    """NaN, infinities, -0, negatives, values above 1, subnormals and the neighbours of rounding ties in every
    channel; test_pvrtc_ref.py pins the twin's bytes for them to literals"""
    src, want = special_source(dtype)
    assert np.array_equal(P.to_rgba8(src), want)
    for fmt in (RGB, RGBA):
        for q in (Quality.Lowest, Quality.Highest):
            got = gpu_ctx.encode_pvrtc([src], make_params(fmt, Type.UNorm, q))[0]
            assert np.array_equal(got, P.encode(src, int(fmt), int(q))), (fmt, q)
            # the same bytes from the literal RGBA8 values: the load pass itself, not only its agreement with the twin
            assert np.array_equal(got, P.encode(want.astype(np.uint8), int(fmt), int(q))), (fmt, q)


@pytest.mark.parametrize("fmt, mask", [(RGB, (0, 0, 0, 1)), (RGB, (0, 0, 0, 0)), (RGBA, (0, 0, 0, 0))])
def test_zero_weight_masks(gpu_ctx, fmt, mask):
    """every candidate's error is 0: kernel and twin must agree on "first minimum" and "keep if not worse\""""
    img = tile_content(32, 32, "graded", 9)
    for q in (Quality.Lowest, Quality.Highest):
        got = gpu_ctx.encode_pvrtc([img], make_params(fmt, Type.UNorm, q, color_mask=mask))[0]
        assert np.array_equal(got, P.encode(img, int(fmt), int(q), mask=mask)), q


# ---- E. one vector per colour field -------------------------------------------------------------------------------
def test_hand_vectors_every_colour_field_on_gpu(gpu_ctx):
    """the expected texels are literals derived by hand in test_pvrtc_ref.py, not computed by the twin"""
    def decode(p, fmt):
        return gpu_ctx.decode_pvrtc(p, Format(fmt), 8, 8)
    for name, word, mod, want in FIELD_VECTORS:
        check_constant_vector(decode, word, mod, want)
    for word, mod, want in TWO_COLOUR_VECTORS:
        check_constant_vector(decode, word, mod, want)


# ---- F. the device SSE entries refuse a misaligned result pointer ------------------------------------------------
def test_sse_device_entries_reject_misaligned_result(gpu_ctx):
    """the kernels add to sse_device with 64-bit atomics: a pointer that is not 8-byte aligned is CFHIP_E_INVALID
    before anything is enqueued (the buffer keeps its fill), and the context goes on working"""
    import torch
    rng = np.random.default_rng(17)
    ref = rng.integers(0, 256, (32, 64, 4), dtype=np.uint8)
    ref_d = torch.from_numpy(ref).to("cuda")
    sse = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    assert sse.data_ptr() % 8 == 0
    torch.cuda.synchronize()              # the context's stream is not torch's: the fill must have landed

    payload = rng.integers(0, 256, P.payload_size(64, 32), dtype=np.uint8)
    blk = torch.from_numpy(payload).to("cuda")
    with pytest.raises(api.CfhipError) as e:
        gpu_ctx.decode_pvrtc_sse_device(blk.data_ptr(), RGBA, 64, 32, ref_d.data_ptr(), 256, sse.data_ptr() + 4)
    assert e.value.code == api.E_INVALID
    torch.cuda.synchronize()
    assert (sse.cpu().numpy() == -1).all()
    gpu_ctx.decode_pvrtc_sse_device(blk.data_ptr(), RGBA, 64, 32, ref_d.data_ptr(), 256, sse.data_ptr() + 8)
    torch.cuda.synchronize()
    assert [int(v) for v in sse.cpu()[1:5]] == P.sse(payload, ref)
    assert int(sse[0]) == -1 and int(sse[5]) == -1

    bc1 = rng.integers(0, 256, api.payload_size(Format.BC1_RGBA, Type.UNorm, 64, 32), dtype=np.uint8)
    blk = torch.from_numpy(bc1).to("cuda")
    sse.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(api.CfhipError) as e:
        gpu_ctx.decode_sse_device(blk.data_ptr(), Format.BC1_RGBA, Type.UNorm, 64, 32, ref_d.data_ptr(), 256,
                                  sse.data_ptr() + 4)
    assert e.value.code == api.E_INVALID
    torch.cuda.synchronize()
    assert (sse.cpu().numpy() == -1).all()
    gpu_ctx.decode_sse_device(blk.data_ptr(), Format.BC1_RGBA, Type.UNorm, 64, 32, ref_d.data_ptr(), 256,
                              sse.data_ptr() + 8)
    torch.cuda.synchronize()
    texels, _ = gpu_ctx.decode(bc1, Format.BC1_RGBA, Type.UNorm, 64, 32)
    assert [int(v) for v in sse.cpu()[1:5]] == exact_sse(texels, ref)
