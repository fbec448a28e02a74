"""The signed distance field from alpha on the GPU (cfhip_alpha_sdf_array_device) against its numpy twin
(tests/alpha_sdf_ref.py), byte for byte: the written channels, the channels left alone, the padding between the rows and
the result records."""
import ctypes

import numpy as np
import pytest

import alpha_sdf_ref as R
from cuttlefish_amd import (CfhipError, ColorSpace, CubeFace, Dimension, Format, Image, ResizeFilter, Texture, Type, api,
                            process_image)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)
WRAPS = [(False, False), (True, False), (False, True), (True, True)]


def content(kind, h, w, dtype, seed=0):
    """(h, w, 4) image of dtype with random colour and alpha: a few discs, sparse single texels, dense with sparse holes,
    soft noise (for the thresholds; 127 and 128 among its 8-bit values), nothing, everything, or one texel"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "discs":
        a = np.zeros((h, w))
        for _ in range(max(2, h*w//600)):
            cy, cx, r = rng.integers(h), rng.integers(w), rng.integers(1, 9)
            a[(x - cx)**2 + (y - cy)**2 <= r*r] = 1.0
    elif kind == "sparse":
        a = (rng.random((h, w)) < 0.02).astype(np.float64)
    elif kind == "holes":
        a = (rng.random((h, w)) < 0.97).astype(np.float64)
    elif kind == "noise":
        a = np.clip(rng.random((h, w))*3.0 - 1.0, 0, 1)
        a.flat[:2] = (127/255, 128/255)
    elif kind == "none":
        a = np.zeros((h, w))
    elif kind == "all":
        a = np.full((h, w), 0.75)
    else:
        a = np.zeros((h, w))
        a[kind[1], kind[0]] = 1.0                          # kind = (x, y)
    img = np.concatenate([rng.random((h, w, 3)), a[..., None]], -1)
    if dtype == np.uint8:
        return np.round(img*255).astype(np.uint8)
    return img.astype(dtype)


def upload(img, pad):
    """the image on the device with `pad` components of 0xFF bytes after each row -> (byte tensor, pitch in bytes)"""
    h, w = img.shape[:2]
    row = w*4*img.itemsize
    buf = np.full((h, row + pad*img.itemsize), 0xFF, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    return torch.from_numpy(buf).cuda(), buf.shape[1]


def download(t, like):
    """-> (the image, the padding bytes)"""
    h, w = like.shape[:2]
    row = w*4*like.itemsize
    b = t.cpu().numpy()
    return b[:, :row].copy().view(like.dtype).reshape(h, w, 4), b[:, row:]


def prefill(h, w, dtype, seed):
    """a destination's content before the call: any bytes that are not NaN patterns worth worrying about"""
    rng = np.random.default_rng(1000 + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    return (rng.random((h, w, 4))*4.0 - 2.0).astype(dtype)


def run(ctx, images, spread, scale=1, out_dtype=None, pad=0, dpad=0, stream=0, in_place=False, **kw):
    """one call on uploaded copies -> (the destinations before it, after it, the records as a structured array)"""
    h, w = images[0].shape[:2]
    out_dtype = images[0].dtype if out_dtype is None else np.dtype(out_dtype)
    src = [upload(im, pad) for im in images]
    before = [im for im in images] if in_place else [prefill(h//scale, w//scale, out_dtype, l) for l in range(len(images))]
    dst = src if in_place else [upload(b, dpad) for b in before]
    res = torch.full((len(images) + 1, 4), -1, dtype=torch.int32, device="cuda")
    ctx.alpha_sdf_device([t.data_ptr() for t, _ in src], api.pixel_type_of(images[0]), w, h, src[0][1],
                         [t.data_ptr() for t, _ in dst], api.pixel_type_of(before[0]), dst[0][1], spread, scale,
                         results=res.data_ptr(), stream=stream, **kw)
    if stream:
        torch.cuda.synchronize()
    outs = []
    for (t, _), b in zip(dst, before):
        out, padding = download(t, b)
        assert (padding == 0xFF).all(), "the bytes between the destination's rows were written"
        outs.append(out)
    if not in_place:
        for (t, _), im in zip(src, images):
            back, padding = download(t, im)
            assert back.tobytes() == im.tobytes() and (padding == 0xFF).all(), "the source was written"
    rec = res.cpu().numpy()
    assert (rec[-1] == -1).all(), "a record past the layers was written"
    return before, outs, rec[:-1].copy().view(api.SDF_RESULT_DTYPE).reshape(-1)


def check(ctx, images, spread, scale=1, **kw):
    """the call against the twin, layer by layer -> the records"""
    before, outs, rec = run(ctx, images, spread, scale, **kw)
    tw = {k: kw[k] for k in ("threshold", "wrap") if k in kw}
    for l, (im, b, out) in enumerate(zip(images, before, outs)):
        values, wrec = R.sdf(im, spread, scale, out_dtype=out.dtype, **tw)
        want = R.apply(b, values, kw.get("channels", "a"))
        assert {k: int(rec[l][k]) for k in R.FIELDS} == wrec, (l, spread, scale, kw)
        assert out.tobytes() == want.tobytes(), (l, spread, scale, kw, int((out != want).any(-1).sum()))
    return rec


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (17, 1), (63, 2), (64, 2), (65, 3), (130, 70), (300, 5)])
def test_shapes_at_scale_1(gpu_ctx, w, h):
    """one texel, one column, one row, a word less one, a word, a word and one, several tiles each way with ragged
    edges, five words of a few rows"""
    for kind in ("discs", "sparse", "holes", (w - 1, h - 1), (0, h//2)):
        for wrap in (False, True):
            check(gpu_ctx, [content(kind, h, w, np.uint8, seed=w + h)], 3, pad=3, dpad=1, wrap=wrap)
    check(gpu_ctx, [content("discs", h, w, np.float32, seed=1)], 16, pad=2)


def test_a_shape_at_scale_16(gpu_ctx):
    for kind in ("discs", "sparse", "holes"):
        for wrap in (False, True):
            check(gpu_ctx, [content(kind, 80, 192, np.uint8, seed=5)], 16, 16, wrap=wrap, dpad=2)


@pytest.mark.parametrize("spread", [1, 3, 16, 126])
def test_spreads(gpu_ctx, spread):
    """126: the window is larger than the surface, and wraps around it more than once"""
    for (w, h), scale in (((130, 70), 1), ((144, 80), 4), ((17, 1), 1), ((1, 17), 1), ((300, 5), 1)):
        for wrap in (False, True):
            rec = check(gpu_ctx, [content("discs", h, w, np.uint8, seed=spread)], spread, scale, wrap=wrap)
            check(gpu_ctx, [content("holes", h, w, np.float16, seed=spread + 1)], spread, scale, wrap=wrap)
        assert 0 < rec[0]["inside"] < w*h


@pytest.mark.parametrize("scale", R.SCALES)
def test_scales(gpu_ctx, scale):
    for w, h in ((64, 32), (144, 80)):
        for kind, spread in (("discs", 8), ("holes", 2), ("sparse", 20)):
            check(gpu_ctx, [content(kind, h, w, np.float32, seed=scale)], spread, scale, out_dtype=np.uint8)


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("threshold", [0.0, 0.5])
def test_wraps_and_thresholds(gpu_ctx, wrap, threshold):
    for dtype, (w, h), scale in ((np.uint8, (37, 21), 1), (np.float16, (72, 132), 4), (np.float32, (130, 70), 1)):
        img = content("noise", h, w, dtype, seed=7)
        rec = check(gpu_ctx, [img], 5, scale, pad=1, wrap=wrap, threshold=threshold)
        assert rec[0]["inside"] == R.inside_mask(img, threshold).sum()
    # inside texels at two corners only: the far side is near with wrap
    edge = content((0, 0), 24, 40, np.float32, 8)
    edge[23, 39, 3] = 1.0
    for scale in (1, 4):
        rec = check(gpu_ctx, [edge], 6, scale, wrap=wrap, threshold=threshold)
        assert rec[0]["inside"] == 2


def test_single_class_surfaces(gpu_ctx):
    for kind, v in (("all", 255), ("none", 0)):
        for (w, h), scale in (((70, 37), 1), ((64, 32), 8)):
            for wrap in (False, True):
                img = content(kind, h, w, np.uint8, 3)
                before, outs, rec = run(gpu_ctx, [img], 4, scale, wrap=wrap)
                assert (outs[0][..., 3] == v).all() and (outs[0][..., :3] == before[0][..., :3]).all()
                assert rec[0]["saturated"] == w*h and rec[0]["inside"] == (w*h if v else 0)
                check(gpu_ctx, [img], 4, scale, wrap=wrap)


def test_nan_and_infinite_alpha(gpu_ctx):
    for dtype in (np.float32, np.float16):
        img = content("discs", 21, 37, dtype, 6)
        img[1, 1, 3] = np.nan
        img[2, 5, 3] = -np.nan
        img[3, 3, 3] = np.inf
        img[4, 4, 3] = -np.inf
        img[20, 36, 3] = np.nan
        img[0, 30:37, 3] = np.inf
        mask = R.inside_mask(img, 0.5)
        assert not mask[1, 1] and not mask[2, 5] and mask[3, 3] and not mask[4, 4]
        rec = check(gpu_ctx, [img], 4, out_dtype=np.float32)
        assert rec[0]["inside"] == mask.sum()
        check(gpu_ctx, [img], 4, threshold=0.0, wrap=True, in_place=True)


@pytest.mark.parametrize("src", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dst", DTYPES, ids=lambda d: np.dtype(d).name)
def test_pixel_type_pairs_with_padded_pitches(gpu_ctx, src, dst):
    for (w, h), scale in (((37, 21), 1), ((72, 40), 4)):
        check(gpu_ctx, [content("discs", h, w, src, seed=w)], 7, scale, out_dtype=dst, pad=5, dpad=3)
        check(gpu_ctx, [content("noise", h, w, src, seed=h)], 2, scale, out_dtype=dst, pad=1, dpad=6, wrap=(True, False))


@pytest.mark.parametrize("channels", ["a", "r", "rgba", "gb"])
def test_channel_masks_leave_the_other_components(gpu_ctx, channels):
    mask = R.channel_mask(channels)
    for dtype in DTYPES:
        for scale in (1, 2):
            img = content("discs", 20, 36, np.uint8, 9)
            before, outs, _ = run(gpu_ctx, [img], 3, scale, out_dtype=dtype, dpad=2, channels=channels)
            for ch in range(4):
                same = outs[0][..., ch].tobytes() == before[0][..., ch].tobytes()
                assert same == (not mask >> ch & 1), (channels, ch)
            check(gpu_ctx, [img], 3, scale, out_dtype=dtype, dpad=2, channels=channels)
    check(gpu_ctx, [img], 3, channels=mask)


def test_five_layers_in_one_call(gpu_ctx):
    w, h = 72, 36
    layers = [content(k, h, w, np.float16, seed=i) for i, k in enumerate(("discs", "none", "sparse", "all", (w - 1, 0)))]
    for scale in (1, 4):
        kw = dict(pad=4, dpad=1, wrap=(True, False), out_dtype=np.uint8)
        rec = check(gpu_ctx, layers, 6, scale, **kw)
        assert rec["inside"].tolist()[1] == 0 and rec["inside"].tolist()[3] == w*h and rec["inside"].tolist()[4] == 1
        assert rec["saturated"].tolist()[1] == rec["saturated"].tolist()[3] == w*h
        # one call of five layers = five calls of one (the destinations are prefilled per layer index: compare alpha)
        _, outs, _ = run(gpu_ctx, layers, 6, scale, **kw)
        for l, im in enumerate(layers):
            _, one, rec1 = run(gpu_ctx, [im], 6, scale, **kw)
            assert one[0][..., 3].tobytes() == outs[l][..., 3].tobytes() and rec1.tobytes() == rec[l:l + 1].tobytes()


def test_in_place_at_scale_1(gpu_ctx):
    for dtype in DTYPES:
        for wrap in (False, True):
            img = content("discs", 70, 130, dtype, 12)
            rec = check(gpu_ctx, [img, content("holes", 70, 130, dtype, 13)], 20, pad=2, wrap=wrap, in_place=True)
            assert rec[0]["inside"] == R.inside_mask(img).sum()
    check(gpu_ctx, [img], 126, in_place=True, channels="rgba")


def test_identical_calls_launch_counts_and_timing(gpu_ctx):
    layers = [content(k, 24, 40, np.uint8, seed=i) for i, k in enumerate(("discs", "sparse", "noise", "holes", "all"))]
    _, a, rec_a = run(gpu_ctx, layers, 9, 4, wrap=True)
    _, b, rec_b = run(gpu_ctx, layers, 9, 4, wrap=True)
    assert rec_a.tobytes() == rec_b.tobytes() and [x.tobytes() for x in a] == [x.tobytes() for x in b]
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_alpha_sdf_column_kernel"
    # 3 launches at scale 1 and 4 above, whatever the layers and the spread
    for scale, launches in ((1, 3), (4, 4), (8, 4)):
        for images in (layers[:1], layers):
            for spread in (1, 126):
                gpu_ctx.profile_begin()
                run(gpu_ctx, images, spread, scale)
                ms, n = gpu_ctx.profile_end()
                assert ms > 0 and n == launches <= 4, (scale, len(images), spread, n)


def test_a_stream_of_the_caller_orders_the_work(gpu_ctx):
    """the content arrives on the caller's stream just before the call and is read back on it just after: the passes
    must run between the two, on that stream"""
    img = content("discs", 72, 136, np.float32, 9)
    values, wrec = R.sdf(img, 12, 4, wrap=(False, True), out_dtype=np.float16)
    s = torch.cuda.Stream()
    dev = torch.zeros((72, 136, 4), dtype=torch.float32, device="cuda")
    low = torch.zeros((18, 34, 4), dtype=torch.float16, device="cuda")
    src = torch.from_numpy(img).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    big = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.zero_()                                        # something in front on the stream
        dev.copy_(src)
        gpu_ctx.alpha_sdf_device([dev.data_ptr()], api.PixelType.RGBA32F, 136, 72, 136*16, [low.data_ptr()],
                                 api.PixelType.RGBA16F, 34*8, 12, 4, wrap=(False, True), channels="ra",
                                 results=res.data_ptr(), stream=s.cuda_stream)
        out = low.clone()
    s.synchronize()
    want = R.apply(np.zeros((18, 34, 4), np.float16), values, "ra")
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert res.cpu().numpy().view(np.uint32).tolist() == [wrec[k] for k in R.FIELDS]
    # and the context's other entries follow on their own stream
    got, rec = gpu_ctx.alpha_sdf(img, 12, 4, wrap=(False, True), channels="ra", out_dtype=np.float16)
    assert got.tobytes() == want.tobytes() and rec == wrec


def test_host_convenience(gpu_ctx):
    for dtype in DTYPES:
        img = content("discs", 24, 40, dtype, 10)
        view = img[:, 4:36]                                # a view: made contiguous
        got, rec = gpu_ctx.alpha_sdf(view, 5, 1, 0.25, (True, False), "a")
        values, wrec = R.sdf(view, 5, 1, 0.25, (True, False))
        assert got.dtype == img.dtype and got.tobytes() == R.apply(view, values).tobytes() and rec == wrec
        got, rec = gpu_ctx.alpha_sdf(view, 5, 8, channels="gb", out_dtype=np.uint8)
        values, wrec = R.sdf(view, 5, 8, out_dtype=np.uint8)
        assert got.shape == (3, 4, 4) and got.tobytes() == R.apply(np.zeros((3, 4, 4), np.uint8), values, "gb").tobytes() and rec == wrec
    with pytest.raises(ValueError):
        gpu_ctx.alpha_sdf(img, 5, threshold=1.0)
    with pytest.raises(ValueError):
        gpu_ctx.alpha_sdf(img[:21], 5, 8)


def test_every_invalid_argument_by_its_text_and_nothing_written(gpu_ctx):
    """straight at the library, past make_sdf_params: every refusal names its argument, and neither the destination nor
    the records change"""
    src = torch.from_numpy(content("discs", 8, 16, np.float32, 11)).cuda()
    dst = torch.full((4, 8, 4), 7.0, dtype=torch.float32, device="cuda")
    res = torch.full((2, 4), -1, dtype=torch.int32, device="cuda")
    ok = dict(src=[src.data_ptr()], dst=[dst.data_ptr()], layers=1, spt=1, dpt=1, w=16, h=8, sp=16*16, dp=8*16, flags=0, t=0.5,
              spread=5, scale=2, mask=8, reserved=0, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        s = (ctypes.c_void_p*max(len(a["src"]), 1))(*a["src"]) if a["src"] is not None else None
        d = (ctypes.c_void_p*max(len(a["dst"]), 1))(*a["dst"]) if a["dst"] is not None else None
        p = api.SdfParams(a["flags"], a["t"], a["spread"], a["scale"], a["mask"], a["reserved"])
        rc = gpu_ctx._lib.cfhip_alpha_sdf_array_device(gpu_ctx._h, s, a["layers"], a["spt"], a["w"], a["h"], a["sp"], d, a["dpt"],
                                                       a["dp"], ctypes.byref(p) if a["params"] else None,
                                                       ctypes.c_void_p(res.data_ptr()), None)
        return rc, gpu_ctx._lib.cfhip_last_error(gpu_ctx._h)
    cases = [(dict(params=False), b"params is NULL"), (dict(src=None), b"src is NULL"), (dict(dst=None), b"dst is NULL"),
             (dict(src=[None]), b"src[0] is NULL"), (dict(dst=[None]), b"dst[0] is NULL"),
             (dict(src=[src.data_ptr() + 2]), b"src[0] not aligned"), (dict(dst=[dst.data_ptr() + 1]), b"dst[0] not aligned"),
             (dict(layers=0), b"layers"), (dict(layers=65536), b"layers"),
             (dict(w=0), b"width and height"), (dict(h=0), b"width and height"), (dict(w=32770, sp=1 << 30), b"width and height"),
             (dict(h=32770), b"width and height"),
             (dict(w=15), b"multiple of the scale"), (dict(h=7), b"multiple of the scale"),
             (dict(scale=0), b"scale"), (dict(scale=3), b"scale"), (dict(scale=32), b"scale"),
             (dict(spread=0), b"spread"), (dict(spread=127), b"spread"),
             (dict(t=-0.5), b"alpha_threshold"), (dict(t=1.0), b"alpha_threshold"), (dict(t=float("nan")), b"alpha_threshold"),
             (dict(flags=4), b"flags"), (dict(mask=0), b"channel_mask"), (dict(mask=16), b"channel_mask"),
             (dict(reserved=1), b"reserved"), (dict(spt=3), b"src_pixel_type"), (dict(dpt=-1), b"dst_pixel_type"),
             (dict(sp=16*16 - 4), b"src_pitch_bytes"), (dict(sp=16*16 + 2), b"src_pitch_bytes"),
             (dict(dp=8*16 - 4), b"dst_pitch_bytes"), (dict(dp=8*16 + 2), b"dst_pitch_bytes"),
             (dict(dst=[src.data_ptr()]), b"in place"), (dict(dst=[src.data_ptr()], scale=1, dpt=2, dp=16*8), b"in place"),
             (dict(w=32768, h=32768, layers=3, sp=32768*16, dp=16384*16, src=[src.data_ptr()]*3, dst=[dst.data_ptr()]*3), b"2^31 texels")]
    for kw, text in cases:
        rc, message = call(**kw)
        assert rc == api.E_INVALID and text in message, (kw, message)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 7.0).all() and (res.cpu().numpy() == -1).all()
    with pytest.raises(CfhipError) as e:
        gpu_ctx.alpha_sdf_device([src.data_ptr()], api.PixelType.RGBA32F, 16, 8, 16*16, [dst.data_ptr()], api.PixelType.RGBA32F,
                                 8*16 - 4, 5, 2)
    assert e.value.code == api.E_INVALID and "dst_pitch_bytes" in str(e.value)
    # and the same call, valid, goes through
    assert call()[0] == 0 and (dst.cpu().numpy()[..., :3] == 7.0).all() and not (dst.cpu().numpy()[..., 3] == 7.0).any()


def test_the_field_magnifies_better_than_box_filtered_alpha(gpu_ctx):
    """the purpose, through the GPU: three 256^2 masks to 32^2 at scale 8 and spread 8 as RGBA8, magnified bilinearly by 8
    and cut at 0.5 -- at most half the wrong texels of the box-filtered alpha on the disc and the bar, fewer on the star"""
    got = {}
    for name, mask in R.shapes().items():
        img = np.zeros(mask.shape + (4,), np.uint8)
        img[..., 3] = mask*255
        out, rec = gpu_ctx.alpha_sdf(img, 8, 8)
        assert out.shape == (32, 32, 4) and out[..., 3].tobytes() == R.sdf(img, 8, 8)[0].tobytes() and rec["inside"] == mask.sum()
        got[name] = (R.mismatches(out[..., 3]/255.0, mask), R.mismatches(R.box_alpha(mask, 8), mask))
        print("%s: field %d, box-filtered alpha %d wrong texels" % ((name,) + got[name]))
    assert 2*got["disc"][0] <= got["disc"][1] and 2*got["bar"][0] <= got["bar"][1]
    assert got["star"][0] < got["star"][1]


def test_image_distance_field():
    img = content("discs", 32, 48, np.uint8, 11)
    im = Image(img, ColorSpace.sRGB)
    f = im.distance_field(6, wrap=(False, True))
    values, _ = R.sdf(img, 6, wrap=(False, True))
    assert isinstance(f, Image) and f.pixels.dtype == np.uint8 and f.pixels.tobytes() == R.apply(img, values).tobytes()
    assert im.pixels.tobytes() == img.tobytes() and f.color_space == ColorSpace.sRGB
    assert f._last is not None and f._last[1] is f.pixels                       # save_bytes reads the device buffer
    assert f.save_bytes() == Image(R.apply(img, values), ColorSpace.sRGB).save_bytes()
    # scale 4: the other channels are the image's own Box resize
    g = im.distance_field(6, 4, 0.25, False, "ga")
    small = im.resize(12, 8, ResizeFilter.Box)
    values, _ = R.sdf(img, 6, 4, 0.25, out_dtype=np.float32)
    assert g.pixels.shape == (8, 12, 4) and g.pixels.dtype == np.float32
    assert g.pixels.tobytes() == R.apply(small.pixels, values, "ga").tobytes()
    fl = Image(content("sparse", 9, 14, np.float32, 12))
    assert fl.distance_field(2, threshold=0.5).pixels.tobytes() == \
        R.apply(fl.pixels, R.sdf(fl.pixels, 2)[0]).tobytes()
    assert Image(np.ones((4, 4, 4), np.float32), rgbf=True).distance_field(2) is None


def test_texture_alpha_distance_field_on_a_cube_with_two_levels():
    t = Texture(Dimension.Cube, 32, 32, 0, 2)
    level0 = [content("discs", 32, 32, np.uint8, f) for f in range(6)]
    level1 = [content("sparse", 16, 16, np.float32, 10 + f) for f in range(6)]
    level1[2] = content("none", 16, 16, np.float32, 12)
    for f in range(6):
        assert t.set_image(level0[f], CubeFace(f), 0) and t.set_image(level1[f], CubeFace(f), 1)
    assert t.sdf_results() == []
    assert t.alpha_distance_field(5, wrap=False, channels="a") is True
    rec = t.sdf_results()
    assert len(rec) == 12 and [(r["mip"], r["face"]) for r in rec] == [(m, f) for m in range(2) for f in range(6)]
    for m, level in enumerate((level0, level1)):
        for f, im in enumerate(level):
            values, wrec = R.sdf(im, 5)
            got = t.get_image(CubeFace(f), m)
            assert got.dtype == im.dtype and got.tobytes() == R.apply(im, values).tobytes(), (m, f)
            r = rec[m*6 + f]
            assert (r["inside"], r["saturated"]) == (wrec["inside"], wrec["saturated"])
    assert rec[6 + 2]["inside"] == 0 and rec[6 + 2]["saturated"] == 256
    assert t.convert(Format.BC3, Type.UNorm)
    assert t.alpha_distance_field(5) is False               # converted


def test_process_image_writes_the_field_over_the_resized_image():
    img = content("discs", 32, 48, np.uint8, 13)
    kw = dict(filter=ResizeFilter.Box)
    ops_only = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 48, 32, **kw)         # the colour-space pass alone
    assert ops_only.shape == (32, 48, 4) and ops_only.dtype == np.float32
    plain = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 8, **kw)
    values, rec = R.sdf(ops_only, 6, 4, 0.25, (True, False))
    assert 0 < rec["inside"] < 32*48
    got = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 8, sdf=dict(spread=6, threshold=0.25, wrap=(True, False), channels="ra"), **kw)
    assert got.shape == (8, 12, 4) and got.tobytes() == R.apply(plain, values, "ra").tobytes() and got.tobytes() != plain.tobytes()
    assert process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 8, sdf=None, **kw).tobytes() == plain.tobytes()
    # nothing resized: at scale 1 after the one ops pass
    same = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 48, 32, sdf=dict(spread=6))
    assert same.tobytes() == R.apply(ops_only, R.sdf(ops_only, 6)[0]).tobytes()
    with pytest.raises(ValueError):
        process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 8, premultiply=True, sdf=dict(spread=6))
    with pytest.raises(ValueError):
        process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 16, 8, sdf=dict(spread=6))      # 3 x 4
