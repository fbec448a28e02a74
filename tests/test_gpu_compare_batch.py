"""The batched compare (cfhip_compare_batch / cfhip_compare_batch_device; csrc/compare.hip, csrc/compare_batch.h)
against the per-surface entry on the same inputs, which tests/test_gpu_compare.py pins to tests/compare_ref.py.
Surface i of a batch must return the very bytes cfhip_compare returns for it alone -- result struct and error map
-- so there is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

from cuttlefish_amd import api, make_params, synth

pytestmark = pytest.mark.gpu

# one (format, type) per kernel family and decoded layout
BC1, BC7, ETC2A, BC4S, BC5, EACRG_S, BC6H, ASTC4, ASTC12x10, ASTC6_HDR = (
    (29, 0), (36, 0), (40, 0), (33, 1), (34, 0), (42, 1), (35, 4), (43, 0), (55, 0), (47, 4))
PAIRS = [BC1, BC7, ETC2A, BC4S, BC5, EACRG_S, BC6H, ASTC4, ASTC12x10, ASTC6_HDR]
IDS = ["bc1", "bc7", "etc2-rgba8", "bc4-snorm", "bc5", "eac-rg11-snorm", "bc6h", "astc4x4", "astc12x10", "astc6x6-hdr"]
LDR_UNORM = [BC1, BC7, ETC2A, BC5, ASTC4, ASTC12x10]

# 1x1, a partial block, one block, no SSIM window (10 < 11), exactly one window, two SSIM tiles across and one
# down, then a 64x64 cube with its whole mip chain: 6 faces x 7 levels = 42 surfaces, in storage order
SMALL = [(1, 1), (3, 5), (4, 4), (10, 40), (11, 11), (27, 26)]
CUBE = [(64 >> m, 64 >> m) for m in range(7) for _ in range(6)]


def _sizes(pair):
    extra = []
    if pair == ASTC6_HDR:
        extra = [(385, 7)]             # 65 blocks across: a block row longer than one 64-block run
    if pair == BC1:
        extra = [(1028, 1024)]         # 257 x 256 blocks = 257 Pass A workgroups: the final fold wraps past thread 255
    return SMALL + extra + CUBE


def _image(pair, w, h, seed):
    """(what the encoder takes, the reference the metrics read)"""
    fmt, typ = pair
    if typ in (4, 5):
        return synth.hdr_probe(w, h, seed=seed, signed=typ == 5)
    img = synth.photo(w, h, seed=seed)
    if typ == 1:
        return ((img.astype(np.float32)/255.0)*2.0 - 1.0).astype(np.float32)
    return img


_CASES = {}


def _case(ctx, pair):
    """sizes, encoder payloads and references of a pair; made once and never changed"""
    if pair not in _CASES:
        sizes = _sizes(pair)
        refs = [_image(pair, w, h, 100 + i) for i, (w, h) in enumerate(sizes)]
        pays = ctx.encode(refs, make_params(pair[0], pair[1], 0))
        for a in refs + pays:
            a.setflags(write=False)
        _CASES[pair] = (sizes, pays, refs)
    return _CASES[pair]


def _bits(r):
    return (r.texels, r.error_blocks, r.channels, r.ssim_windows,
            np.array(r.sse + r.log_sse + r.ssim + r.ref_max).tobytes(),
            None if r.block_errors is None else r.block_errors.tobytes())


def _alone(ctx, pair, pays, refs, **kw):
    return [ctx.compare(p, r, pair[0], pair[1], **kw) for p, r in zip(pays, refs)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _bits(g) == _bits(w), (i, g.texels, g.sse, w.sse, g.ssim, w.ssim)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_batch_returns_the_bytes_of_the_per_surface_entry(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    want = _alone(gpu_ctx, pair, pays, refs, ssim=True, block_map=True)
    got = gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], ssim=True, block_map=True)
    _assert_same(got, want)
    assert gpu_ctx.last_kernel_name() == ("cfhip_compare_batch_astc_kernel" if pair[0] >= 43
                                          else "cfhip_compare_batch_block_kernel")
    hdr = pair[1] == 4
    for (w, h), g in zip(sizes, got):
        assert g.texels == w*h
        windows = 0 if hdr or w < 11 or h < 11 else (w - 10)*(h - 10)
        assert g.ssim_windows == windows, (w, h)
        assert all(np.isnan(g.ssim[c]) == (windows == 0) for c in g.compared()), (w, h)
        assert all(np.isnan(v) for v in g.log_sse[:1]) == (not hdr)
    # two identical batched calls return identical bytes
    _assert_same(gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], ssim=True, block_map=True), got)
    # without the SSIM pass, and without maps
    _assert_same(gpu_ctx.compare_batch(pays, refs, pair[0], pair[1]), _alone(gpu_ctx, pair, pays, refs))


@pytest.mark.parametrize("pair", LDR_UNORM, ids=[IDS[PAIRS.index(p)] for p in LDR_UNORM])
def test_random_payloads_count_error_blocks_per_surface(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    rng = np.random.default_rng(7*pair[0] + 1)
    keep = [i for i, (w, h) in enumerate(sizes) if w*h <= 64*64]
    rnd = [rng.integers(0, 256, pays[i].size, dtype=np.uint8) for i in keep]
    rrefs = [refs[i] for i in keep]
    want = _alone(gpu_ctx, pair, rnd, rrefs, ssim=True, block_map=True)
    _assert_same(gpu_ctx.compare_batch(rnd, rrefs, pair[0], pair[1], ssim=True, block_map=True), want)
    if pair[0] >= 43:
        # random ASTC blocks are mostly illegal: the counts differ from surface to surface
        assert len({r.error_blocks for r in want}) > 2


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["rgba16f", "rgba32f"])
@pytest.mark.parametrize("pair", [BC7, ASTC12x10, BC6H], ids=["bc7", "astc12x10", "bc6h"])
def test_reference_types(gpu_ctx, pair, dtype):
    sizes, pays, refs = _case(gpu_ctx, pair)
    if refs[0].dtype == np.uint8:
        refs = [(r.astype(np.float32)/np.float32(255.0)).astype(dtype) for r in refs]
    else:
        refs = [r.astype(dtype) for r in refs]
    want = _alone(gpu_ctx, pair, pays, refs, ssim=True, block_map=True)
    _assert_same(gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], ssim=True, block_map=True), want)


@pytest.mark.parametrize("pair", [BC7, BC5, ASTC4, BC6H], ids=["bc7", "bc5", "astc4x4", "bc6h"])
def test_mask(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    mask = (1, 0, 1, 0)
    want = _alone(gpu_ctx, pair, pays, refs, mask=mask, ssim=True, block_map=True)
    got = gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], mask=mask, ssim=True, block_map=True)
    _assert_same(got, want)
    assert {g.channels for g in got} == {0b0001 if pair == BC5 else 0b0101}
    # nothing left to compare: no SSIM pass at all, as for a single surface
    none = gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], mask=(0, 0, 0, 0), ssim=True)
    _assert_same(none, _alone(gpu_ctx, pair, pays, refs, mask=(0, 0, 0, 0), ssim=True))
    assert all(g.channels == 0 and g.ssim_windows == 0 for g in none)


def _device_batch(ctx, pair, pays, refs, pitch_pad=0, maps=None, mask=None, ssim=True, stream=None, stagger=0):
    """The device form.  pitch_pad: extra bytes per reference row; maps: indices of the surfaces that get an error
    map (None: all); stagger: bytes between payloads, so that they are not block-aligned.  Returns a function that
    downloads the Comparisons (call it once the stream is done)."""
    import torch
    fmt, typ = pair
    bw, bh, _ = api.query(fmt, typ)
    n = len(pays)
    pix = {np.uint8: 0, np.float32: 1, np.float16: 2}[refs[0].dtype.type]
    tb = refs[0].dtype.itemsize*4
    boffs, o = [], 0
    for p in pays:
        boffs.append(o)
        o += p.nbytes + stagger
    blob = np.zeros(o + 16, np.uint8)
    for p, bo in zip(pays, boffs):
        blob[bo:bo + p.nbytes] = p
    roffs, pitches, o = [], [], 0
    for r in refs:
        h, w = r.shape[:2]
        o = (o + 15)//16*16 + (tb if pitch_pad else 0)       # padded rows start off 16-byte alignment too
        roffs.append(o)
        pitches.append(w*tb + pitch_pad)
        o += h*pitches[-1]
    rblob = np.full(o + 16, 0x5A, np.uint8)
    for r, ro, pitch in zip(refs, roffs, pitches):
        h, w = r.shape[:2]
        rblob[ro:ro + h*pitch].reshape(h, pitch)[:, :w*tb] = np.ascontiguousarray(r).view(np.uint8).reshape(h, w*tb)
    grids = [((r.shape[0] + bh - 1)//bh, (r.shape[1] + bw - 1)//bw) for r in refs]
    maps = list(range(n)) if maps is None else list(maps)
    moffs, o = {}, 0
    for i in maps:
        moffs[i] = o
        o += grids[i][0]*grids[i][1]
    size = ctypes.sizeof(api.CompareResult)
    d_blob, d_ref = torch.from_numpy(blob).cuda(), torch.from_numpy(rblob).cuda()
    d_map = torch.full((max(o, 1),), -7.0, dtype=torch.float32, device="cuda")
    d_res = torch.zeros(n*size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    surfaces = []
    for i, r in enumerate(refs):
        s = dict(blocks=d_blob.data_ptr() + boffs[i], ref=d_ref.data_ptr() + roffs[i], width=r.shape[1],
                 height=r.shape[0], ref_pitch_bytes=pitches[i])
        if i in moffs:
            s.update(block_errors=d_map.data_ptr() + 4*moffs[i], block_errors_capacity=grids[i][0]*grids[i][1])
        surfaces.append(s)
    ctx.compare_batch_device(surfaces, fmt, typ, pix, d_res.data_ptr(), mask=mask, ssim=ssim,
                             stream=stream.cuda_stream if stream is not None else 0)
    layout, _ = api.decoded_layout(fmt, typ)

    def fetch():
        keep = (d_blob, d_ref)                                # alive until the results are read
        raw, emap = d_res.cpu().numpy(), d_map.cpu().numpy()
        out = []
        for i in range(n):
            res = api.CompareResult.from_buffer_copy(raw[i*size:(i + 1)*size].tobytes())
            m = None
            if i in moffs:
                m = emap[moffs[i]:moffs[i] + grids[i][0]*grids[i][1]].reshape(grids[i]).copy()
            out.append(api.Comparison(res, layout, m))
        del keep
        return out
    return fetch


@pytest.mark.parametrize("pair", [BC1, EACRG_S, ASTC6_HDR], ids=["bc1", "eac-rg11-snorm", "astc6x6-hdr"])
def test_host_form_equals_device_form(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    host = gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], ssim=True, block_map=True)
    _assert_same(_device_batch(gpu_ctx, pair, pays, refs)(), host)


@pytest.mark.parametrize("pair", [BC7, ASTC12x10], ids=["bc7", "astc12x10"])
def test_pitches_neither_tight_nor_16_byte_aligned_and_maps_on_some_surfaces(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    want = _alone(gpu_ctx, pair, pays, refs, ssim=True, block_map=True)
    some = [i for i in range(len(pays)) if i % 3 == 1]
    # device form: RGBA8 rows 4 bytes longer than tight, starting 4 bytes off 16-byte alignment, payloads staggered
    got = _device_batch(gpu_ctx, pair, pays, refs, pitch_pad=4, maps=some, stagger=3)()
    for i, (g, w) in enumerate(zip(got, want)):
        assert _bits(g)[:5] == _bits(w)[:5], i
        assert (g.block_errors is not None) == (i in some)
        if i in some:
            assert g.block_errors.tobytes() == w.block_errors.tobytes(), i
    # host form: rows 7 bytes longer than tight (views into wider arrays)
    wide = []
    for r in refs:
        h, w = r.shape[:2]
        buf = np.zeros((h, w*4 + 7), np.uint8)
        buf[:, :w*4] = r.reshape(h, w*4)
        wide.append(buf)
    n = len(pays)
    surf = (api.CompareSurface*n)()
    emaps = {i: np.full(want[i].block_errors.shape, -7.0, np.float32) for i in some}
    for i, (p, b, r) in enumerate(zip(pays, wide, refs)):
        surf[i].blocks, surf[i].blocks_bytes = p.ctypes.data, p.nbytes
        surf[i].width, surf[i].height = r.shape[1], r.shape[0]
        surf[i].ref, surf[i].ref_pitch_bytes = b.ctypes.data, b.strides[0]
        if i in emaps:
            surf[i].block_errors, surf[i].block_errors_capacity = emaps[i].ctypes.data, emaps[i].size
    res = (api.CompareResult*n)()
    gpu_ctx._check(gpu_ctx._lib.cfhip_compare_batch(gpu_ctx._h, pair[0], pair[1], surf, n, 0, None, api.COMPARE_SSIM,
                                                    ctypes.addressof(res)))
    layout, _ = api.decoded_layout(*pair)
    for i in range(n):
        g = api.Comparison(res[i], layout, emaps.get(i))
        assert _bits(g)[:5] == _bits(want[i])[:5], i
        if i in emaps:
            assert emaps[i].tobytes() == want[i].block_errors.tobytes(), i


def test_batch_on_a_callers_stream_then_a_per_surface_call(gpu_ctx):
    """Lease ordering: the batch on a caller's stream returns with its work queued, its tables and scratch in the
    context's staging; the per-surface call that follows on the context's stream uses the same staging."""
    import torch
    sizes, pays, refs = _case(gpu_ctx, BC1)
    want = _alone(gpu_ctx, BC1, pays, refs, ssim=True, block_map=True)
    big = sizes.index((1028, 1024))
    s = torch.cuda.Stream()
    fetch = _device_batch(gpu_ctx, BC1, pays, refs, stream=s)
    after = gpu_ctx.compare(pays[big], refs[big], 29, 0, ssim=True, block_map=True)
    again = gpu_ctx.compare_batch(pays[:7], refs[:7], 29, 0, ssim=True, block_map=True)
    s.synchronize()
    _assert_same(fetch(), want)
    assert _bits(after) == _bits(want[big])
    _assert_same(again, want[:7])


@pytest.mark.parametrize("pair", [BC7, ASTC4], ids=["bc7", "astc4x4"])
def test_launch_count_does_not_depend_on_the_number_of_surfaces(gpu_ctx, pair):
    sizes, pays, refs = _case(gpu_ctx, pair)
    first = len(SMALL)                                      # the 42 surfaces of the cube chain; its first is 64 x 64
    for ssim, launches in ((False, 2), (True, 4)):
        counts = []
        for n in (1, 42):
            gpu_ctx.profile_begin()
            gpu_ctx.compare_batch(pays[first:first + n], refs[first:first + n], pair[0], pair[1], ssim=ssim,
                                  block_map=True)
            ms, k = gpu_ctx.profile_end()
            assert ms > 0.0
            counts.append(k)
        assert counts == [launches, launches], (ssim, counts)
    # no surface with a valid window: the SSIM flag adds no launch
    gpu_ctx.profile_begin()
    gpu_ctx.compare_batch(pays[:4], refs[:4], pair[0], pair[1], ssim=True)
    assert gpu_ctx.profile_end()[1] == 2
    # outside a profile the call's own launches are what last_kernel_ms sums
    gpu_ctx.compare_batch(pays, refs, pair[0], pair[1], ssim=True)
    assert gpu_ctx.last_kernel_ms() > 0.0
