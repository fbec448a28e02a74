"""Alpha bleeding on the GPU (cfhip_alpha_bleed_array_device) against its numpy twin (tests/alpha_bleed_ref.py), byte for
byte: the pixels, the padding between the rows and the result records."""
import numpy as np
import pytest

import alpha_bleed_ref as R
from cuttlefish_amd import (CfhipError, ColorSpace, CubeFace, Dimension, Format, Image, ResizeFilter, Texture, Type, api,
                            process_image)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)


def content(kind, h, w, dtype, seed=0):
    """(h, w, 4) image of dtype with random colour everywhere -- under the transparent texels too -- and alpha: a few
    opaque discs, sparse single texels, soft noise (for the thresholds; 127 and 128 among its 8-bit values), nothing,
    everything, or one texel"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "discs":
        a = np.zeros((h, w))
        for _ in range(max(2, h*w//400)):
            cy, cx, r = rng.integers(h), rng.integers(w), rng.integers(1, 5)
            a[(x - cx)**2 + (y - cy)**2 <= r*r] = 1.0
    elif kind == "sparse":
        a = (rng.random((h, w)) < 0.02).astype(np.float64)
        a[rng.integers(h), rng.integers(w)] = 1.0
    elif kind == "noise":
        a = np.clip(rng.random((h, w))*3.0 - 1.5, 0, 1)
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


def run(ctx, images, pad=0, stream=0, **kw):
    """one call on uploaded copies -> (the images after it, the records as a structured array)"""
    h, w = images[0].shape[:2]
    dev = [upload(im, pad) for im in images]
    res = torch.full((len(images) + 1, 4), -1, dtype=torch.int32, device="cuda")
    ctx.alpha_bleed_device([t.data_ptr() for t, _ in dev], api.pixel_type_of(images[0]), w, h, dev[0][1], results=res.data_ptr(),
                           stream=stream, **kw)
    if stream:
        torch.cuda.synchronize()
    outs = []
    for (t, _), im in zip(dev, images):
        out, padding = download(t, im)
        assert (padding == 0xFF).all(), "the bytes between the rows were written"
        outs.append(out)
    rec = res.cpu().numpy()
    assert (rec[-1] == -1).all(), "a record past the layers was written"
    return outs, rec[:-1].copy().view(api.BLEED_RESULT_DTYPE).reshape(-1)


def check(ctx, images, pad=0, **kw):
    """the call against the twin, layer by layer -> the records"""
    outs, rec = run(ctx, images, pad, **kw)
    for l, (im, out) in enumerate(zip(images, outs)):
        want, wrec = R.bleed(im, kw.get("threshold", 0.0), kw.get("wrap", False), kw.get("max_distance", 0))
        assert {k: int(rec[l][k]) for k in R.FIELDS} == wrec, (l, kw)
        assert out.tobytes() == want.tobytes(), (l, kw, int((out != want).any(-1).sum()) if out.dtype == np.uint8 else None)
    return rec


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("w,h", [(37, 21), (64, 64)])
def test_pixel_types_with_a_padded_pitch(gpu_ctx, dtype, w, h):
    img = content("discs", h, w, dtype, seed=w)
    rec = check(gpu_ctx, [img], pad=5)
    assert 0 < rec[0]["seeds"] < w*h and rec[0]["filled"] == w*h - rec[0]["seeds"]
    check(gpu_ctx, [content("sparse", h, w, dtype, seed=h)], pad=1, wrap=True)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (17, 1), (300, 5), (130, 70)])
def test_shapes(gpu_ctx, w, h):
    """one texel, one column, one row, P far above one side, several workgroups each way with ragged edges"""
    for kind in ("sparse", (w - 1, h - 1), (0, h//2), "none"):
        for wrap in (False, True):
            check(gpu_ctx, [content(kind, h, w, np.uint8, seed=w + h)], pad=3, wrap=wrap)
    check(gpu_ctx, [content("discs", h, w, np.float32, seed=1)], pad=2)


@pytest.mark.parametrize("wrap", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("max_distance", [0, 3])
@pytest.mark.parametrize("threshold", [0.0, 0.5])
def test_wrap_max_distance_and_threshold(gpu_ctx, wrap, max_distance, threshold):
    for dtype, (w, h) in ((np.uint8, (37, 21)), (np.float16, (70, 130))):
        img = content("noise", h, w, dtype, seed=7)
        rec = check(gpu_ctx, [img], pad=1, wrap=wrap, max_distance=max_distance, threshold=threshold)
        assert rec[0]["seeds"] == R.seed_mask(img, threshold).sum() and rec[0]["max_dist2"] <= (9 if max_distance else 1 << 31)
    # seeds at the edges only: the far side is near with wrap, and max_distance cuts the fill
    edge = content((0, 0), 21, 37, np.float32, 8)
    edge[20, 36, 3] = 1.0
    rec = check(gpu_ctx, [edge], wrap=wrap, max_distance=max_distance, threshold=threshold)
    assert rec[0]["seeds"] == 2 and (rec[0]["filled"] < 37*21 - 2) == bool(max_distance)


def test_five_layers_in_one_call(gpu_ctx):
    w, h = 70, 37
    layers = [content(k, h, w, np.float16, seed=i) for i, k in enumerate(("discs", "none", "sparse", "all", (w - 1, 0)))]
    rec = check(gpu_ctx, layers, pad=4, wrap=(True, False))
    assert rec["seeds"].tolist()[1] == 0 and rec["seeds"].tolist()[3] == w*h and rec["seeds"].tolist()[4] == 1
    assert rec["filled"].tolist()[1] == rec["filled"].tolist()[3] == 0 and rec["filled"].tolist()[4] == w*h - 1
    # one call of five layers = five calls of one
    outs, _ = run(gpu_ctx, layers, wrap=(True, False))
    for l, im in enumerate(layers):
        one, rec1 = run(gpu_ctx, [im], wrap=(True, False))
        assert one[0].tobytes() == outs[l].tobytes() and rec1.tobytes() == rec[l:l + 1].tobytes()


def test_corner_seed_and_ties(gpu_ctx):
    corner = content((0, 0), 8, 16, np.uint8, 3)
    assert check(gpu_ctx, [corner])[0]["max_dist2"] == 15**2 + 7**2
    assert check(gpu_ctx, [corner], wrap=True)[0]["max_dist2"] == 8**2 + 4**2
    outs, _ = run(gpu_ctx, [corner])
    assert (outs[0][..., :3] == corner[0, 0, :3]).all()
    # two seeds equally far: the smaller seed word (x | y << 16) wins
    tie = content((1, 2), 5, 9, np.float32, 4)
    tie[2, 7, 3] = 1.0
    check(gpu_ctx, [tie])
    outs, _ = run(gpu_ctx, [tie])
    assert outs[0][2, 4, :3].tobytes() == tie[2, 1, :3].tobytes() and outs[0][2, 5, :3].tobytes() == tie[2, 7, :3].tobytes()
    diag = content((3, 0), 6, 6, np.uint8, 5)
    diag[3, 0, 3] = 255
    check(gpu_ctx, [diag])
    outs, _ = run(gpu_ctx, [diag])
    assert outs[0][0, 0, :3].tolist() == diag[0, 3, :3].tolist()


def test_bits_are_copied_and_nan_alpha_is_no_seed(gpu_ctx):
    img = content((4, 2), 4, 6, np.float32, 6)
    img[2, 4, :3] = np.array([0x7FA00001, 0x80000000, 0x00000001], np.uint32).view(np.float32)
    img[1, 1, 3] = np.nan
    img[3, 3, 3] = -1.0
    rec = check(gpu_ctx, [img])
    assert rec[0]["seeds"] == 1 and rec[0]["filled"] == 23
    half = content((1, 1), 3, 5, np.float16, 7)
    half[1, 1, :3] = np.array([0x7E01, 0x8000, 0x0001], np.uint16).view(np.float16)
    half[0, 0, 3] = np.nan
    check(gpu_ctx, [half])


def test_identical_calls_launch_counts_and_timing(gpu_ctx):
    layers = [content(k, 21, 37, np.uint8, seed=i) for i, k in enumerate(("discs", "sparse", "noise"))]
    a, rec_a = run(gpu_ctx, layers, threshold=0.5, wrap=True)
    b, rec_b = run(gpu_ctx, layers, threshold=0.5, wrap=True)
    assert rec_a.tobytes() == rec_b.tobytes() and [x.tobytes() for x in a] == [x.tobytes() for x in b]
    assert gpu_ctx.last_kernel_ms() > 0 and gpu_ctx.last_kernel_name() == "cfhip_alpha_bleed_step_kernel"
    # 2 + log2(P) launches, whatever the layers
    for images, launches in ((layers[:1], 8), (layers, 8), ([content("discs", 1, 1, np.uint8)], 2),
                             ([content("discs", 5, 300, np.uint8)], 11)):
        gpu_ctx.profile_begin()
        run(gpu_ctx, images)
        ms, n = gpu_ctx.profile_end()
        assert ms > 0 and n == launches


def test_a_stream_of_the_caller_orders_the_work(gpu_ctx):
    """the content arrives on the caller's stream just before the call and is read back on it just after: the passes
    must run between the two, on that stream"""
    img = content("discs", 70, 130, np.float32, 9)
    want, wrec = R.bleed(img)
    s = torch.cuda.Stream()
    dev = torch.zeros((70, 130, 4), dtype=torch.float32, device="cuda")
    src = torch.from_numpy(img).cuda()
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    big = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.zero_()                                        # something in front on the stream
        dev.copy_(src)
        gpu_ctx.alpha_bleed_device([dev.data_ptr()], api.PixelType.RGBA32F, 130, 70, 130*16, results=res.data_ptr(),
                                   stream=s.cuda_stream)
        out = dev.clone()
    s.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert res.cpu().numpy().view(np.uint32).tolist() == [wrec[k] for k in R.FIELDS]
    # and the context's other entries follow on their own stream
    got, rec = gpu_ctx.alpha_bleed(img)
    assert got.tobytes() == want.tobytes() and rec == wrec


def test_host_convenience_and_errors(gpu_ctx):
    for dtype in DTYPES:
        img = content("discs", 21, 37, dtype, 10)
        got, rec = gpu_ctx.alpha_bleed(img[:, 3:30], 0.25, (True, False), 6)      # a view: made contiguous
        want, wrec = R.bleed(img[:, 3:30], 0.25, (True, False), 6)
        assert got.dtype == img.dtype and got.tobytes() == want.tobytes() and rec == wrec
    with pytest.raises(CfhipError) as e:
        gpu_ctx.alpha_bleed(img, threshold=1.0)
    assert e.value.code == api.E_INVALID and "alpha_threshold" in str(e.value)


def test_image_bleed_alpha_then_save_bytes():
    img = content("discs", 21, 37, np.uint8, 11)
    want, _ = R.bleed(img, 0.0, (False, True))
    im = Image(img, ColorSpace.sRGB)
    assert im.bleed_alpha(wrap=(False, True)) is True
    assert im.pixels.dtype == np.uint8 and im.pixels.tobytes() == want.tobytes()
    assert im._last is not None and im._last[1] is im.pixels                   # save_bytes reads the device buffer
    assert im.save_bytes() == Image(want, ColorSpace.sRGB).save_bytes()
    assert im.save_bytes() != Image(img, ColorSpace.sRGB).save_bytes()
    f = Image(content("sparse", 9, 14, np.float32, 12))
    assert f.bleed_alpha(0.5, max_distance=2) and f.pixels.tobytes() == R.bleed(content("sparse", 9, 14, np.float32, 12), 0.5, False, 2)[0].tobytes()
    assert Image(np.ones((4, 4, 4), np.float32), rgbf=True).bleed_alpha() is False


def test_texture_bleed_alpha_on_a_cube_with_two_levels():
    t = Texture(Dimension.Cube, 32, 32, 0, 2)
    level0 = [content("discs", 32, 32, np.uint8, f) for f in range(6)]
    level1 = [content("sparse", 16, 16, np.float32, 10 + f) for f in range(6)]
    level1[2] = content("none", 16, 16, np.float32, 12)
    for f in range(6):
        assert t.set_image(level0[f], CubeFace(f), 0) and t.set_image(level1[f], CubeFace(f), 1)
    assert t.bleed_results() == []
    assert t.bleed_alpha(wrap=False) is True
    rec = t.bleed_results()
    assert len(rec) == 12 and [(r["mip"], r["face"]) for r in rec] == [(m, f) for m in range(2) for f in range(6)]
    for m, level in enumerate((level0, level1)):
        for f, im in enumerate(level):
            want, wrec = R.bleed(im)
            got = t.get_image(CubeFace(f), m)
            assert got.dtype == im.dtype and got.tobytes() == want.tobytes(), (m, f)
            r = rec[m*6 + f]
            assert (r["seeds"], r["filled"], r["max_dist2"]) == (wrec["seeds"], wrec["filled"], wrec["max_dist2"])
    assert rec[6 + 2]["seeds"] == 0 and rec[6 + 2]["filled"] == 0
    assert t.convert(Format.BC3, Type.UNorm)
    assert t.bleed_alpha() is False                         # converted


def test_process_image_bleeds_between_the_ops_and_the_resize():
    img = content("discs", 20, 24, np.uint8, 13)
    kw = dict(filter=ResizeFilter.Box)
    ops_only = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 24, 20, **kw)         # the colour-space pass alone
    assert ops_only.shape == (20, 24, 4) and ops_only.dtype == np.float32
    bled, rec = R.bleed(ops_only, 0.5, (True, False), 5)
    assert 0 < rec["filled"] < 20*24 - rec["seeds"]
    want = process_image(bled, ColorSpace.Linear, ColorSpace.Linear, 12, 10, **kw)           # the resize alone
    got = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, bleed=dict(threshold=0.5, wrap=(True, False), max_distance=5), **kw)
    plain = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, **kw)
    assert got.shape == (10, 12, 4) and got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes()
    assert process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, bleed=None, **kw).tobytes() == plain.tobytes()
    # nothing resized: after the one ops pass
    same = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 24, 20, bleed=dict(threshold=0.5, wrap=(True, False), max_distance=5))
    assert same.tobytes() == bled.tobytes()
    with pytest.raises(ValueError):
        process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, premultiply=True, bleed={})


def test_bleeding_removes_the_fringe_from_the_mips():
    """the purpose, end to end: opaque discs over black transparent texels, a Box chain with and without bleeding; the
    visible texels of levels 1 and 2 against the alpha-weighted colour of the level-0 texels under them"""
    rng = np.random.default_rng(14)
    y, x = np.mgrid[0:64, 0:64]
    base = np.zeros((64, 64, 4), np.float32)
    colour = (0.35 + 0.6*rng.random(3)*np.ones((64, 64, 3)) + 0.05*np.sin(x/5.0)[..., None]).astype(np.float32)
    for _ in range(9):
        cy, cx, r = rng.integers(64), rng.integers(64), rng.integers(3, 9)
        disc = (x - cx)**2 + (y - cy)**2 <= r*r
        base[disc, :3] = colour[disc]
        base[disc, 3] = 1.0
    assert 0.05 < base[..., 3].mean() < 0.8 and not base[base[..., 3] == 0][:, :3].any()
    plain, bled = Texture(64, 64), Texture(64, 64)
    assert plain.set_image(base) and bled.set_image(base.copy())
    assert bled.bleed_alpha() and plain.generate_mipmaps(ResizeFilter.Box) and bled.generate_mipmaps(ResizeFilter.Box)
    assert plain.mip_level_count() == bled.mip_level_count() == 7
    for k in range(7):
        assert plain.get_image(k)[..., 3].tobytes() == bled.get_image(k)[..., 3].tobytes(), k
    b64 = base.astype(np.float64)
    for k in (1, 2):
        n = 64 >> k
        blocks = b64.reshape(n, 1 << k, n, 1 << k, 4)
        wsum = blocks[..., 3].sum((1, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = (blocks[..., :3]*blocks[..., 3:]).sum((1, 3))/wsum[..., None]
        visible = plain.get_image(k)[..., 3] > 0.25
        assert visible.any() and (wsum[visible] > 0).all()
        err = [float(((t.get_image(k)[..., :3].astype(np.float64) - ref)[visible]**2).sum()) for t in (plain, bled)]
        print("level %d: squared error of %d visible texels, plain %.6g, bled %.6g" % (k, visible.sum(), err[0], err[1]))
        assert err[1] < err[0], (k, err)
