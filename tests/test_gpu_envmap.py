"""The environment-map entries on the GPU against their numpy twin (tests/envmap_ref.py): the panorama pass within a bound
derived from the taps it read -- the two sides call different atan2 and asin -- and the prefiltered chain and the nine
coefficients byte for byte."""
import ctypes

import numpy as np
import pytest

import envmap_ref as R
from cuttlefish_amd import CfhipError, CubeFace, Dimension, FileType, Format, SaveResult, Texture, Type, api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)


def panorama(h, w, dtype, seed=0, sun=False):
    """(h, w, 4) of dtype: smooth light with noise on it; sun: 0.01 everywhere but one texel of 1e5"""
    rng = np.random.default_rng(seed)
    if sun:
        img = np.full((h, w, 4), 0.01)
        img[h//3, (2*w)//3] = 1.0e5
    else:
        y, x = np.mgrid[0:h, 0:w]
        img = (0.5 + 0.4*np.sin(x*2.0*np.pi/w + 1.0)*np.cos(y*np.pi/h))[..., None]*np.array([1.0, 0.7, 0.4, 1.0])
        img = np.clip(img + 0.2*rng.random((h, w, 4)), 0.0, 1.0)
    if dtype == np.uint8:
        return np.round(img*255).astype(np.uint8)
    return img.astype(dtype)


def upload(img, pad=0):
    """the image on the device with `pad` components of 0xFF bytes after each row -> (byte tensor, pitch in bytes)"""
    h, w = img.shape[:2]
    row = w*4*img.itemsize
    buf = np.full((h, row + pad*img.itemsize), 0xFF, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    return torch.from_numpy(buf).cuda(), buf.shape[1]


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def to_cube(ctx, img, n, q=None, pad=0, stream=0):
    """the six faces of one call on an uploaded copy, the source checked untouched -> (6, n, n, 4) float32"""
    dev, pitch = upload(img, pad)
    out = torch.full((6, n, n, 4), -7.0, dtype=torch.float32, device="cuda")
    kw = {} if q is None else dict(supersample=q)
    ctx.equirect_to_cube_device(dev.data_ptr(), api.pixel_type_of(img), img.shape[1], img.shape[0], pitch,
                                [out[f].data_ptr() for f in range(6)], n, stream=stream, **kw)
    if stream:
        torch.cuda.synchronize()
    back = dev.cpu().numpy()
    row = img.shape[1]*4*img.itemsize
    assert back[:, :row].tobytes() == np.ascontiguousarray(img).tobytes() and (back[:, row:] == 0xFF).all()
    return out.cpu().numpy()


def check_cube(got, img, n, q):
    """|gpu - twin| <= ulp32(twin) + 2 * 2^-40 * max(W, H) * R, R the spread of the taps read -> (share of identical
    values, the largest difference)"""
    want, spread = R.equirect_to_cube(img, n, 2 if q is None else q)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = ulp32(want) + 2.0*2.0**-40*max(img.shape[0], img.shape[1])*spread
    assert np.isfinite(got).all() and (diff <= bound).all(), (img.shape, n, q, float((diff - bound).max()))
    return float((got == want).mean()), float(diff.max())


SHAPES = [((4, 2), 1, None), ((7, 3), 2, None), ((7, 3), 3, 2), ((64, 32), 5, 1), ((64, 32), 16, 4), ((130, 70), 33, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("size,n,q", SHAPES)
def test_panorama_to_cube_against_the_twin(gpu_ctx, size, n, q, dtype):
    img = panorama(size[1], size[0], dtype, seed=n)
    same, worst = check_cube(to_cube(gpu_ctx, img, n, q), img, n, q)
    print("%dx%d %s -> %d^2 q=%s: %.4f of the values bit-identical, largest difference %.3g" % (size + (np.dtype(dtype).name, n, q, same, worst)))


def test_a_padded_pitch_and_a_sun_beside_darkness(gpu_ctx):
    for dtype in (np.float32, np.float16):
        img = panorama(32, 64, np.float32, sun=True)
        if dtype == np.float16:
            img = np.minimum(img, np.float32(60000.0)).astype(dtype)    # 1e5 is no half: as bright as one gets
        got = to_cube(gpu_ctx, img, 16, 2, pad=5)
        same, worst = check_cube(got, img, 16, 2)
        assert got.max() > 100.0 and got.min() == np.float32(R.to_float(img).min())
        print("sun %s: %.4f bit-identical, largest difference %.3g" % (np.dtype(dtype).name, same, worst))
    img = panorama(32, 64, np.uint8, seed=3)
    check_cube(to_cube(gpu_ctx, img, 16, 2, pad=3), img, 16, 2)


def test_host_convenience_of_the_panorama(gpu_ctx):
    img = panorama(16, 32, np.float32, seed=4)
    faces = gpu_ctx.equirect_to_cube(img[:, 2:30], 4)      # a view: made contiguous
    assert len(faces) == 6 and faces[0].shape == (4, 4, 4) and faces[0].dtype == np.float32
    check_cube(np.stack(faces), np.ascontiguousarray(img[:, 2:30]), 4, 2)
    with pytest.raises(ValueError):
        gpu_ctx.equirect_to_cube(img, 4, supersample=3)
    with pytest.raises(ValueError):
        gpu_ctx.equirect_to_cube(img, 0)


# ---- the chain ---------------------------------------------------------------------------------------------------------
def cube(n, seed, hdr=True):
    rng = np.random.default_rng(seed)
    f = rng.random((6, n, n, 4))
    return (f*f*(40.0 if hdr else 1.0)).astype(np.float32)


def box_chain(ctx, faces, levels):
    """the first `levels` levels of the Box chain as the library builds it -> a list of (6, m, m, 4) float32 tensors"""
    n = faces.shape[1]
    chain = [torch.from_numpy(np.ascontiguousarray(faces)).cuda()]
    chain += [torch.empty((6, max(1, n >> l), max(1, n >> l), 4), dtype=torch.float32, device="cuda") for l in range(1, levels)]
    if levels > 1:
        ctx.generate_mips_array_device([chain[0][f].data_ptr() for f in range(6)], api.PixelType.RGBA32F, n, n, n*16,
                                       [[chain[l][f].data_ptr() for l in range(1, levels)] for f in range(6)],
                                       filter=int(api.ResizeFilter.Box))
    return chain


def run_prefilter(ctx, chain, tables, stream=0):
    """one call on a device chain -> the destination levels as numpy, the sources checked untouched"""
    n, L, K = chain[0].shape[1], len(chain), len(tables)
    before = [c.cpu().numpy() for c in chain]
    out = [torch.full((6, max(1, n >> k), max(1, n >> k), 4), -7.0, dtype=torch.float32, device="cuda") for k in range(K)]
    ctx.cube_prefilter_device([[chain[l][f].data_ptr() for l in range(L)] for f in range(6)], n,
                              [[out[k][f].data_ptr() for k in range(K)] for f in range(6)], tables, stream=stream)
    if stream:
        torch.cuda.synchronize()
    assert all(c.cpu().numpy().tobytes() == b.tobytes() for c, b in zip(chain, before)), "a source level was written"
    return [o.cpu().numpy() for o in out], before


def same_bytes_or_both_nan(got, want):
    """IEEE leaves the sign and payload of a NaN that an operation makes to the implementation: a NaN of the twin is any
    NaN here, every other value is its bytes"""
    nan = np.isnan(want)
    return (np.isnan(got) == nan).all() and got[~nan].tobytes() == want[~nan].tobytes()


def tables_for(n, L, roughness, samples):
    return [None if r == 0.0 else R.ggx_sample_table(r, samples, n, L) for r in roughness]


@pytest.mark.parametrize("n,full,samples,K", [(1, True, 64, 1), (2, True, 128, 2), (3, False, 64, 2), (3, True, 1024, 2),
                                              (5, False, 128, 3), (5, True, 64, 3), (16, True, 64, 5), (16, False, 128, 1)])
def test_prefilter_is_the_twin_byte_for_byte(gpu_ctx, n, full, samples, K):
    """every size of the issue, one source level or the full chain, the three table sizes; the last level of a full chain
    is roughness 1 on the 1 x 1 face, the first of a full chain roughness 0, a copy"""
    L = api.cube_level_count(n) if full else 1
    chain = box_chain(gpu_ctx, cube(n, seed=n + samples), L)
    roughness = R.default_roughness(K) if K > 1 else [0.35]
    if not full:
        roughness[0] = 0.15                                # a single source level: level 0 filtered too
    tables = tables_for(n, L, roughness, samples)
    got, src = run_prefilter(gpu_ctx, chain, tables)
    want = R.prefilter(src, tables)
    for k in range(K):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (n, L, samples, k, roughness[k])
    if full and K > 1:
        assert got[0].tobytes() == src[0].tobytes()        # roughness 0: the bits of the source level
        assert got[-1].shape[1] == max(1, n >> (K - 1)) and roughness[-1] == 1.0


def test_a_table_with_one_weighted_record_and_a_copy_of_every_level(gpu_ctx):
    n = 5
    chain = box_chain(gpu_ctx, cube(n, 21), 3)
    table = R.ggx_sample_table(0.7, 64, n, 3)
    table[:, 2] = 0.0
    table[17, 2] = 0.625
    got, src = run_prefilter(gpu_ctx, chain, [table, None, table])
    want = R.prefilter(src, [table, None, table])
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and got[1].tobytes() == src[1].tobytes()
    # one record of weight w: the texel is that record's blend of two fetches times w, over w
    assert np.isfinite(got[0]).all() and got[0].min() >= 0
    got, src = run_prefilter(gpu_ctx, chain, [None, None, None])
    assert all(g.tobytes() == s.tobytes() for g, s in zip(got, src))


def test_nan_and_infinity_in_a_source_texel_propagate_as_the_twin_says(gpu_ctx):
    n = 5
    faces = cube(n, 22)
    faces[2, 1, 3, 0] = np.nan
    faces[4, 4, 0, 1] = np.inf
    faces[1, 0, 0, 2] = -np.inf
    chain = box_chain(gpu_ctx, faces, 1)
    tables = tables_for(n, 1, [0.3, 1.0], 64)
    got, src = run_prefilter(gpu_ctx, chain, tables)
    want = R.prefilter(src, tables)
    for g, w in zip(got, want):
        assert same_bytes_or_both_nan(g, w)
        assert np.isnan(w[..., 0]).any() and np.isfinite(w[..., 3]).all() and not np.isnan(w[..., 0]).all()


def test_host_convenience_of_the_chain(gpu_ctx):
    faces = cube(8, 23)
    levels = gpu_ctx.cube_prefilter([faces[f] for f in range(6)], [0.0, 0.5, 1.0], samples=64)
    chain = box_chain(gpu_ctx, faces, 4)
    tables = [None] + [api.ggx_sample_table(r, 64, 8, 4) for r in (0.5, 1.0)]
    want = R.prefilter([c.cpu().numpy() for c in chain], tables)
    assert [l.shape for l in levels] == [(6, 8, 8, 4), (6, 4, 4, 4), (6, 2, 2, 4)]
    assert all(l.tobytes() == w.tobytes() for l, w in zip(levels, want))
    with pytest.raises(ValueError):
        gpu_ctx.cube_prefilter([faces[f] for f in range(6)], [0.0]*5, samples=64)
    with pytest.raises(ValueError):
        gpu_ctx.cube_prefilter([faces[f] for f in range(6)], [0.5], samples=100)


# ---- the nine coefficients ---------------------------------------------------------------------------------------------
def run_sh9(ctx, faces, stream=0):
    dev = torch.from_numpy(np.ascontiguousarray(faces)).cuda()
    res = torch.full((38,), -7.0, dtype=torch.float64, device="cuda")
    ctx.cube_sh9_device([dev[f].data_ptr() for f in range(6)], faces.shape[1], res.data_ptr(), stream=stream)
    if stream:
        torch.cuda.synchronize()
    rec = res.cpu().numpy()
    assert rec[37] == -7.0 and dev.cpu().numpy().tobytes() == faces.tobytes()
    return rec[:37]


@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_sh9_is_the_twin_byte_for_byte(gpu_ctx, n):
    """one texel, a part of a wavefront, exactly one, one and a texel"""
    faces = cube(n, 30 + n)
    got = run_sh9(gpu_ctx, faces)
    assert got.tobytes() == R.sh9(faces).tobytes()
    coeffs, omega = gpu_ctx.cube_sh9([faces[f] for f in range(6)])
    assert coeffs.shape == (9, 4) and coeffs.tobytes() == got[:36].tobytes() and omega == got[36]
    assert abs(omega - 4.0*np.pi) <= 4.0*np.pi/(n*n)


def test_identical_calls_launch_counts_and_timing(gpu_ctx):
    img = panorama(32, 64, np.float32, seed=5)
    a, b = to_cube(gpu_ctx, img, 16, 2), to_cube(gpu_ctx, img, 16, 2)
    assert a.tobytes() == b.tobytes()
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_equirect_to_cube_kernel"
    chain = box_chain(gpu_ctx, a, 5)
    tables = tables_for(16, 5, [0.0, 0.3, 0.6, 1.0], 64)
    first, second = run_prefilter(gpu_ctx, chain, tables)[0], run_prefilter(gpu_ctx, chain, tables)[0]
    assert [x.tobytes() for x in first] == [x.tobytes() for x in second]
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_cube_prefilter_kernel"
    assert run_sh9(gpu_ctx, a).tobytes() == run_sh9(gpu_ctx, a).tobytes()
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_cube_sh9_rows_kernel"
    # one launch for the six faces; one per destination level, a copy included; two for the coefficients
    for q in (1, 4):
        gpu_ctx.profile_begin()
        to_cube(gpu_ctx, img, 16, q)
        assert gpu_ctx.profile_end()[1] == 1
    for K in (1, 2, 4):
        gpu_ctx.profile_begin()
        run_prefilter(gpu_ctx, chain, tables[:K])
        ms, launches = gpu_ctx.profile_end()
        assert ms > 0 and launches == K
    for faces in (a, cube(3, 6)):
        gpu_ctx.profile_begin()
        run_sh9(gpu_ctx, faces)
        assert gpu_ctx.profile_end()[1] == 2


def test_a_stream_of_the_caller_orders_the_work(gpu_ctx):
    """the panorama arrives on the caller's stream just before the three calls and their results are read back on it just
    after: faces, chain and coefficients must be made between the two, in order, on that stream"""
    img = panorama(32, 64, np.float32, seed=7)
    n = 8
    s = torch.cuda.Stream()
    src = torch.from_numpy(img).cuda()
    dev = torch.zeros((32, 64, 4), dtype=torch.float32, device="cuda")
    faces = torch.zeros((6, n, n, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((6, n, n, 4), dtype=torch.float32, device="cuda")
    res = torch.zeros(37, dtype=torch.float64, device="cuda")
    big = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
    table = R.ggx_sample_table(0.4, 64, n, 1)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.zero_()                                        # something in front on the stream
        dev.copy_(src)
        gpu_ctx.equirect_to_cube_device(dev.data_ptr(), api.PixelType.RGBA32F, 64, 32, 64*16, [faces[f].data_ptr() for f in range(6)],
                                        n, 2, stream=s.cuda_stream)
        gpu_ctx.cube_prefilter_device([[faces[f].data_ptr()] for f in range(6)], n, [[out[f].data_ptr()] for f in range(6)],
                                      [table], stream=s.cuda_stream)
        gpu_ctx.cube_sh9_device([out[f].data_ptr() for f in range(6)], n, res.data_ptr(), stream=s.cuda_stream)
        got_faces, got_out, got_res = faces.clone(), out.clone(), res.clone()
    s.synchronize()
    got_faces = got_faces.cpu().numpy()
    check_cube(got_faces, img, n, 2)
    want = R.prefilter_level([got_faces], n, table)
    assert got_out.cpu().numpy().tobytes() == want.tobytes()
    assert got_res.cpu().numpy().tobytes() == R.sh9(want).tobytes()
    # and the context's other entries follow on their own stream
    assert np.stack(gpu_ctx.equirect_to_cube(img, n)).tobytes() == got_faces.tobytes()


def test_every_invalid_argument_by_its_text_and_nothing_written(gpu_ctx):
    """straight at the library on a live context: every refusal names its argument, and no destination changes"""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    err = lambda: lib.cfhip_last_error(h)                  # noqa: E731
    pano = torch.from_numpy(panorama(4, 8, np.float32)).cuda()
    faces = torch.full((6, 4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    small = torch.full((6, 2, 2, 4), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((2, 6, 4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    res = torch.full((37,), 7.0, dtype=torch.float64, device="cuda")
    fp = [faces[f].data_ptr() for f in range(6)]
    table = R.ggx_sample_table(0.5, 64, 4, 2)

    def arr(values):
        return (ctypes.c_void_p*len(values))(*values) if values is not None else None

    def equirect(**kw):
        a = dict(dict(src=pano.data_ptr(), pt=1, w=8, h=4, pitch=8*16, faces=fp, n=4, q=2), **kw)
        return lib.cfhip_equirect_to_cube_device(h, a["src"], a["pt"], a["w"], a["h"], a["pitch"], arr(a["faces"]), a["n"], a["q"], None)

    def prefilter(**kw):
        a = dict(dict(src=[p for f in range(6) for p in (faces[f].data_ptr(), small[f].data_ptr())], n=4, L=2,
                      dst=[p for f in range(6) for p in (out[0, f].data_ptr(), out[1, f].data_ptr())], K=2,
                      tables=[None, table], counts=[0, 64]), **kw)
        keep = [None if t is None else np.ascontiguousarray(t, np.float32) for t in a["tables"]]
        return lib.cfhip_cube_prefilter_device(h, arr(a["src"]), a["n"], a["L"], arr(a["dst"]), a["K"],
                                               arr([None if t is None else t.ctypes.data for t in keep]),
                                               (ctypes.c_uint32*len(a["counts"]))(*a["counts"]), None)

    def sh9(**kw):
        a = dict(dict(faces=fp, n=4, res=res.data_ptr()), **kw)
        return lib.cfhip_cube_sh9_device(h, arr(a["faces"]), a["n"], a["res"], None)
    nan_table = table.copy()
    nan_table[3, 0] = np.nan
    cases = [(equirect, dict(src=None), b"src is NULL"), (equirect, dict(w=1), b"width is 2 to"), (equirect, dict(h=0), b"width is 2 to"),
             (equirect, dict(w=32769, pitch=1 << 30), b"width is 2 to"), (equirect, dict(pt=3), b"src_pixel_type"),
             (equirect, dict(pitch=8*16 - 4), b"src_pitch_bytes"), (equirect, dict(pitch=8*16 + 2), b"src_pitch_bytes"),
             (equirect, dict(src=pano.data_ptr() + 2), b"src not aligned"), (equirect, dict(q=3), b"supersample"),
             (equirect, dict(q=0), b"supersample"), (equirect, dict(faces=None), b"faces is NULL"), (equirect, dict(n=0), b"face_size"),
             (equirect, dict(n=8193), b"face_size"), (equirect, dict(faces=fp[:5] + [None]), b"faces[5] is NULL"),
             (equirect, dict(faces=[fp[0] + 4] + fp[1:]), b"faces[0] not aligned"),
             (equirect, dict(faces=[pano.data_ptr()] + fp[1:]), b"faces[0] equals src"),
             (prefilter, dict(src=None), b"src_levels is NULL"), (prefilter, dict(dst=None), b"dst_levels is NULL"),
             (prefilter, dict(n=0), b"face_size"), (prefilter, dict(L=0), b"source_levels"), (prefilter, dict(L=4), b"source_levels"),
             (prefilter, dict(K=0), b"dst_count"), (prefilter, dict(K=4), b"dst_count"),
             (prefilter, dict(counts=[0, 32]), b"table_samples[1]"), (prefilter, dict(counts=[0, 4160]), b"table_samples[1]"),
             (prefilter, dict(tables=[None, None]), b"tables[1] is NULL"), (prefilter, dict(tables=[None, nan_table]), b"tables[1][3]"),
             (prefilter, dict(dst=[fp[0]] + [out[1, 0].data_ptr()] + [p for f in range(1, 6) for p in (out[0, f].data_ptr(), out[1, f].data_ptr())]),
              b"dst_levels[0][0] equals src_levels[0][0]"),
             (prefilter, dict(L=1, src=fp, tables=[table, None], counts=[64, 0]), b"a copy"),
             (sh9, dict(faces=None), b"faces is NULL"), (sh9, dict(n=0), b"face_size"), (sh9, dict(faces=[None] + fp[1:]), b"faces[0] is NULL"),
             (sh9, dict(faces=fp[:3] + [fp[3] + 8] + fp[4:]), b"faces[3] not aligned"), (sh9, dict(res=None), b"result_device is NULL"),
             (sh9, dict(res=res.data_ptr() + 4), b"result_device not aligned")]
    for call, kw, text in cases:
        rc = call(**kw)
        assert rc == api.E_INVALID and text in err(), (kw, err())
    torch.cuda.synchronize()
    for t in (faces, small, out, res):
        assert (t.cpu().numpy() == 7.0).all()
    with pytest.raises(CfhipError) as e:
        gpu_ctx.equirect_to_cube_device(pano.data_ptr(), api.PixelType.RGBA32F, 8, 4, 8*16, fp, 4, 3)
    assert e.value.code == api.E_INVALID and "supersample" in str(e.value)
    # and the same calls, valid, go through
    assert equirect() == 0 and sh9() == 0 and not (faces.cpu().numpy() == 7.0).any() and not (res.cpu().numpy() == 7.0).any()
    small.copy_(faces[:, ::2, ::2])
    assert prefilter() == 0 and not (out.cpu().numpy()[0] == 7.0).any()
    level1 = out.cpu().numpy()[1].reshape(6, -1)
    assert not (level1[:, :16] == 7.0).any() and (level1[:, 16:] == 7.0).all()


# ---- the texture -------------------------------------------------------------------------------------------------------
def test_texture_from_panorama_to_a_bc6h_dds_and_back(gpu_ctx):
    img = (panorama(32, 64, np.float32, seed=8)*np.float32(6.0)).astype(np.float32)
    n = 16
    t = Texture.from_panorama(img, n)
    assert t is not None and t.dimension() == Dimension.Cube and t.face_count() == 6 and t.mip_level_count() == 1
    level0 = np.stack([t.get_image(CubeFace(f), 0) for f in range(6)])
    check_cube(level0, img, n, 2)
    sh = t.irradiance_sh9()
    assert sh.shape == (9, 4) and sh.tobytes() == R.sh9(level0)[:36].tobytes()
    # a constant environment of the mean would be lit by about pi times it
    assert np.abs(api.sh9_irradiance(sh, np.array([0.0, 1.0, 0.0]))/np.pi - level0.mean((0, 1, 2))).max() < 0.5*level0.max()
    assert t.prefilter_environment(samples=64) is True and t.mip_level_count() == 5 and t.images_complete()
    chain = [c.cpu().numpy() for c in box_chain(gpu_ctx, level0, 5)]
    tables = [None] + [api.ggx_sample_table(r, 64, n, 5) for r in R.default_roughness(5)[1:]]
    want = R.prefilter(chain, tables)
    for k in range(5):
        got = np.stack([t.get_image(CubeFace(f), k) for f in range(6)])
        assert got.dtype == np.float32 and got.tobytes() == want[k].tobytes(), k
    assert t.convert(Format.BC6H, Type.UFloat)
    assert t.prefilter_environment() is False and t.irradiance_sh9() is None     # converted
    result, data = t.save_bytes(FileType.DDS)
    assert result == SaveResult.Success and len(data) > 6*(16 + 4 + 1 + 1 + 1)*16
    back = Texture.load(data, FileType.DDS)
    assert back is not None and back.dimension() == Dimension.Cube and back.face_count() == 6 and back.mip_level_count() == 5
    assert back.format() == Format.BC6H and back.width(0) == n and back.width(4) == 1
    # fewer levels and a roughness list of one's own
    u = Texture.from_panorama(img.astype(np.float16), 8, supersample=1)
    assert u.prefilter_environment(mip_levels=2, samples=64, roughness=[0.25, 0.75]) and u.mip_level_count() == 2
    assert u.get_image(CubeFace.NegZ, 1).shape == (4, 4, 4)
    assert u.prefilter_environment(roughness=[0.5]) is False and u.prefilter_environment(mip_levels=2, roughness=[0.0, 1.5]) is False
