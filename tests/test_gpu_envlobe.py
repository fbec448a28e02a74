"""The BRDF lookup table, the irradiance cube and the Charlie and Lambert lobes on the GPU against their numpy twin
(tests/envlobe_ref.py): the GGX columns, the irradiance cube and the prefiltered levels byte for byte, the sheen column
within one float32 unit -- its pow is the device library's."""
import ctypes
import functools

import numpy as np
import pytest

import envlobe_ref as E
import envmap_ref as R
from cuttlefish_amd import CfhipError, CubeFace, Dimension, FileType, Format, SaveResult, Texture, Type, api
from test_gpu_envmap import box_chain, cube, run_prefilter, same_bytes_or_both_nan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def run_lut(ctx, w, h, table, sheen, stream=0):
    """one call into a surface with a guard texel after it -> (h, w, 4) float32"""
    out = torch.full((h*w + 1, 4), -7.0, dtype=torch.float32, device="cuda")
    ctx.brdf_lut_device(out.data_ptr(), w, h, table, sheen, stream=stream)
    if stream:
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[h*w] == -7.0).all()
    return got[:h*w].reshape(h, w, 4)


@functools.lru_cache(maxsize=None)
def twin_lut(w, h, samples):
    return E.brdf_lut(w, h, E.hammersley_table(samples), sheen=True)


# 15 texels: no multiple of the four wavefronts of a workgroup; 192: no power of two; 1088: the 1024-record chunk and a
# remainder; 4096: four full chunks
LUT_CASES = [(5, 3, 64), (8, 4, 192), (7, 2, 1088), (16, 16, 4096)]


@pytest.mark.parametrize("w,h,samples", LUT_CASES)
def test_lookup_table_is_the_twin(gpu_ctx, w, h, samples):
    table = E.hammersley_table(samples)
    want = twin_lut(w, h, samples)
    got = run_lut(gpu_ctx, w, h, table, True)
    assert got[..., :2].tobytes() == want[..., :2].tobytes()               # no library call in the GGX columns
    assert (got[..., 3] == 1.0).all()
    b, wb = got[..., 2], want[..., 2]
    differing = int((b != wb).sum())
    print("%dx%d S=%d: %d of %d sheen values differ from the twin" % (w, h, samples, differing, b.size))
    assert (np.abs(b.astype(np.float64) - wb.astype(np.float64)) <= np.spacing(np.maximum(np.abs(b), np.abs(wb)))).all()
    plain = run_lut(gpu_ctx, w, h, table, False)
    assert (plain[..., 2] == 0.0).all() and not np.signbit(plain[..., 2]).any()
    assert plain[..., :2].tobytes() == want[..., :2].tobytes() and (plain[..., 3] == 1.0).all()


@functools.lru_cache(maxsize=None)
def sh9_source():
    return cube(5, 41)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_irradiance_cube_is_the_twin_byte_for_byte(gpu_ctx, n):
    """the record goes from cube_sh9_device to cube_irradiance_device on the device"""
    faces = sh9_source()
    dev = torch.from_numpy(faces).cuda()
    res = torch.zeros(37, dtype=torch.float64, device="cuda")
    gpu_ctx.cube_sh9_device([dev[f].data_ptr() for f in range(6)], 5, res.data_ptr())
    record = res.cpu().numpy()
    assert record.tobytes() == R.sh9(faces).tobytes()
    for over_pi in (False, True):
        out = torch.full((6*n*n + 1, 4), -7.0, dtype=torch.float32, device="cuda")
        size = n*n*16
        gpu_ctx.cube_irradiance_device(res.data_ptr(), [out.data_ptr() + f*size for f in range(6)], n, over_pi)
        got = out.cpu().numpy()
        assert (got[6*n*n] == -7.0).all() and res.cpu().numpy().tobytes() == record.tobytes()
        assert got[:6*n*n].reshape(6, n, n, 4).tobytes() == E.cube_irradiance(record, n, over_pi).tobytes(), (n, over_pi)


@pytest.mark.parametrize("samples", [64, 1088])
@pytest.mark.parametrize("kind", [E.LOBE_CHARLIE, E.LOBE_LAMBERT])
def test_charlie_and_lambert_levels_are_the_prefilter_twin_byte_for_byte(gpu_ctx, kind, samples):
    """the existing kernel is a generic lobe consumer: a full chain of an 8^2 cube, level 0 a copy"""
    n, L = 8, 4
    chain = box_chain(gpu_ctx, cube(n, 50 + kind), L)
    tables = [None] + [E.lobe_sample_table(kind, r, samples, n, L) for r in (0.5, 0.75, 1.0)]
    assert all(t[:, 2].any() for t in tables[1:])
    got, src = run_prefilter(gpu_ctx, chain, tables)
    assert got[0].tobytes() == src[0].tobytes()
    for k in range(1, L):
        want = R.prefilter_level(src, n >> k, tables[k])
        assert got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), (kind, samples, k)
        assert np.isfinite(got[k]).all()


def test_identical_calls_launch_counts_and_timing(gpu_ctx):
    table = api.hammersley_table(192)
    a, b = run_lut(gpu_ctx, 9, 7, table, True), run_lut(gpu_ctx, 9, 7, table, True)
    assert a.tobytes() == b.tobytes()
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_brdf_lut_kernel"
    for sheen in (False, True):
        gpu_ctx.profile_begin()
        run_lut(gpu_ctx, 9, 7, table, sheen)
        ms, launches = gpu_ctx.profile_end()
        assert ms > 0 and launches == 1
    coeffs = R.sh9(sh9_source())[:36].reshape(9, 4)
    first, second = gpu_ctx.cube_irradiance(coeffs, 5), gpu_ctx.cube_irradiance(coeffs, 5)
    assert first.tobytes() == second.tobytes()
    assert gpu_ctx.last_kernel_ms() >= 0 and gpu_ctx.last_kernel_name() == "cfhip_cube_irradiance_kernel"
    for n in (1, 70):                                      # one workgroup a face, and two across with a ragged edge
        gpu_ctx.profile_begin()
        gpu_ctx.cube_irradiance(coeffs, n, over_pi=True)
        assert gpu_ctx.profile_end()[1] == 1


def test_host_conveniences_agree_with_the_device_forms(gpu_ctx):
    table = api.hammersley_table(128)
    assert gpu_ctx.brdf_lut(6, 4, 128, sheen=True).tobytes() == run_lut(gpu_ctx, 6, 4, table, True).tobytes()
    assert gpu_ctx.brdf_lut(6, 4, 128).tobytes() == run_lut(gpu_ctx, 6, 4, table, False).tobytes()
    record = R.sh9(sh9_source())
    for over_pi in (False, True):
        got = gpu_ctx.cube_irradiance(record[:36].reshape(9, 4), 3, over_pi)
        assert got.shape == (6, 3, 3, 4) and got.tobytes() == E.cube_irradiance(record, 3, over_pi).tobytes()
    # fewer channels: the others are 0
    rgb = gpu_ctx.cube_irradiance(record[:36].reshape(9, 4)[:, :3], 3)
    assert rgb[..., :3].tobytes() == E.cube_irradiance(record, 3)[..., :3].tobytes() and (rgb[..., 3] == 0).all()
    faces = cube(8, 52)
    levels = gpu_ctx.cube_prefilter_lobe([faces[f] for f in range(6)], api.LOBE_CHARLIE, [0.0, 0.5, None, 1.0], samples=64)
    chain = box_chain(gpu_ctx, faces, 4)
    tables = [None, api.lobe_sample_table(api.LOBE_CHARLIE, 0.5, 64, 8, 4), None, api.lobe_sample_table(api.LOBE_CHARLIE, 1.0, 64, 8, 4)]
    want = R.prefilter([c.cpu().numpy() for c in chain], tables)
    assert [l.shape for l in levels] == [(6, 8, 8, 4), (6, 4, 4, 4), (6, 2, 2, 4), (6, 1, 1, 4)]
    assert all(l.tobytes() == w.tobytes() for l, w in zip(levels, want))
    ggx = gpu_ctx.cube_prefilter_lobe([faces[f] for f in range(6)], api.LOBE_GGX, [0.0, 0.5], samples=64)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ggx, gpu_ctx.cube_prefilter([faces[f] for f in range(6)], [0.0, 0.5], 64)))
    with pytest.raises(ValueError):                        # no record above the horizon: refused, not a face of NaN
        gpu_ctx.cube_prefilter_lobe([faces[f] for f in range(6)], api.LOBE_CHARLIE, [0.0, 0.2], samples=256)
    with pytest.raises(ValueError):
        gpu_ctx.brdf_lut(0, 4)
    with pytest.raises(ValueError):
        gpu_ctx.brdf_lut(4, 4, samples=100)
    with pytest.raises(ValueError):
        gpu_ctx.cube_irradiance(np.zeros((8, 4)), 4)


def test_a_stream_of_the_caller_orders_the_work(gpu_ctx):
    """the cube arrives on the caller's stream just before the calls and the results are read back on it just after: the
    coefficients, the irradiance cube and the lookup table must be made between the two, in order, on that stream"""
    n, m = 8, 5
    faces = cube(n, 53)
    table = E.hammersley_table(64)
    s = torch.cuda.Stream()
    src = torch.from_numpy(faces).cuda()
    dev = torch.zeros((6, n, n, 4), dtype=torch.float32, device="cuda")
    res = torch.zeros(37, dtype=torch.float64, device="cuda")
    out = torch.zeros((6, m, m, 4), dtype=torch.float32, device="cuda")
    lut = torch.zeros((3, 5, 4), dtype=torch.float32, device="cuda")
    big = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big.zero_()                                        # something in front on the stream
        dev.copy_(src)
        gpu_ctx.cube_sh9_device([dev[f].data_ptr() for f in range(6)], n, res.data_ptr(), stream=s.cuda_stream)
        gpu_ctx.cube_irradiance_device(res.data_ptr(), [out[f].data_ptr() for f in range(6)], m, True, stream=s.cuda_stream)
        gpu_ctx.brdf_lut_device(lut.data_ptr(), 5, 3, table, True, stream=s.cuda_stream)
        got_out, got_lut = out.clone(), lut.clone()
    s.synchronize()
    assert got_out.cpu().numpy().tobytes() == E.cube_irradiance(R.sh9(faces), m, True).tobytes()
    assert got_lut.cpu().numpy()[..., :2].tobytes() == twin_lut(5, 3, 64)[..., :2].tobytes()
    # and the context's other entries follow on their own stream
    assert gpu_ctx.brdf_lut(5, 3, 64, sheen=True).tobytes() == got_lut.cpu().numpy().tobytes()


def test_every_invalid_argument_by_its_text_and_nothing_written(gpu_ctx):
    """straight at the library on a live context: every refusal names its argument, and no destination changes"""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    err = lambda: lib.cfhip_last_error(h)                  # noqa: E731
    lut = torch.full((4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    faces = torch.full((6, 4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    res = torch.full((37,), 7.0, dtype=torch.float64, device="cuda")
    fp = [faces[f].data_ptr() for f in range(6)]
    table = E.hammersley_table(64)
    bad_table = table.copy()
    bad_table[3, 2] = 1.0

    def arr(values):
        return (ctypes.c_void_p*len(values))(*values) if values is not None else None

    def brdf(**kw):
        a = dict(dict(dst=lut.data_ptr(), w=4, h=4, table=table, S=64, sheen=1), **kw)
        t = None if a["table"] is None else np.ascontiguousarray(a["table"], np.float32)
        return lib.cfhip_brdf_lut_device(h, a["dst"], a["w"], a["h"], None if t is None else t.ctypes.data, a["S"], a["sheen"], None)

    def irradiance(**kw):
        a = dict(dict(rec=res.data_ptr(), faces=fp, n=4, over_pi=0), **kw)
        return lib.cfhip_cube_irradiance_device(h, a["rec"], arr(a["faces"]), a["n"], a["over_pi"], None)
    cases = [(brdf, dict(dst=None), b"dst is NULL"), (brdf, dict(dst=lut.data_ptr() + 8), b"dst not aligned"),
             (brdf, dict(w=0), b"width and height are 1 to 1024"), (brdf, dict(h=1025), b"width and height are 1 to 1024"),
             (brdf, dict(table=None), b"table is NULL"), (brdf, dict(S=32), b"samples is"), (brdf, dict(S=100), b"samples is"),
             (brdf, dict(S=4160), b"samples is"), (brdf, dict(sheen=2), b"sheen is 0 or 1"), (brdf, dict(table=bad_table), b"table[3]"),
             (irradiance, dict(rec=None), b"sh9_result_device is NULL"), (irradiance, dict(rec=res.data_ptr() + 4), b"sh9_result_device not aligned"),
             (irradiance, dict(faces=None), b"faces is NULL"), (irradiance, dict(n=0), b"face_size"), (irradiance, dict(n=8193), b"face_size"),
             (irradiance, dict(faces=fp[:2] + [None] + fp[3:]), b"faces[2] is NULL"),
             (irradiance, dict(faces=fp[:5] + [fp[5] + 4]), b"faces[5] not aligned"),
             (irradiance, dict(faces=[res.data_ptr()] + fp[1:]), b"faces[0] equals sh9_result_device"),
             (irradiance, dict(over_pi=3), b"over_pi is 0 or 1")]
    for call, kw, text in cases:
        rc = call(**kw)
        assert rc == api.E_INVALID and text in err(), (kw, err())
    torch.cuda.synchronize()
    for t in (lut, faces, res):
        assert (t.cpu().numpy() == 7.0).all()
    with pytest.raises(CfhipError) as e:
        gpu_ctx.brdf_lut_device(lut.data_ptr(), 4, 2000, table)
    assert e.value.code == api.E_INVALID and "width and height" in str(e.value)
    # and the same calls, valid, go through
    assert brdf() == 0 and irradiance() == 0
    assert not (lut.cpu().numpy() == 7.0).any() and not (faces.cpu().numpy() == 7.0).any() and (res.cpu().numpy() == 7.0).all()


# ---- the texture -------------------------------------------------------------------------------------------------------
def test_texture_lookup_table_to_half_floats_and_a_file(gpu_ctx):
    t = Texture.brdf_lut(32, 256, sheen=True)
    assert t is not None and t.dimension() == Dimension.Dim2D and t.width(0) == t.height(0) == 32 and t.mip_level_count() == 1
    image = t.get_image(0)
    assert image.dtype == np.float32 and image.tobytes() == gpu_ctx.brdf_lut(32, 32, 256, sheen=True).tobytes()
    assert image[..., :2].tobytes() == twin_lut(32, 32, 256)[..., :2].tobytes()
    assert t.convert(Format.R16G16B16A16, Type.Float)
    result, data = t.save_bytes(FileType.DDS)
    assert result == SaveResult.Success and len(data) > 32*32*8
    back = Texture.load(data, FileType.DDS)
    assert back is not None and back.format() == Format.R16G16B16A16 and back.width(0) == 32
    assert Texture.brdf_lut(8, 64).get_image(0)[..., 2].max() == 0.0


def test_texture_irradiance_cube_to_a_bc6h_dds_and_lobe_chains(gpu_ctx):
    n = 16
    faces = cube(n, 54)
    t = Texture(Dimension.Cube, n, n)
    for f in range(6):
        assert t.set_image(faces[f], CubeFace(f))
    record = R.sh9(faces)
    irr = t.irradiance_cube(4)
    assert irr is not None and irr.dimension() == Dimension.Cube and irr.face_count() == 6 and irr.width(0) == 4
    got = np.stack([irr.get_image(CubeFace(f), 0) for f in range(6)])
    assert got.tobytes() == E.cube_irradiance(record, 4, True).tobytes()
    # the sampled form: level 2 of the chain under the uniform table, near the nine coefficients' answer
    lam = t.irradiance_cube(4, method="lambert", samples=256)
    sampled = np.stack([lam.get_image(CubeFace(f), 0) for f in range(6)])
    chain = [c.cpu().numpy() for c in box_chain(gpu_ctx, faces, 5)]
    assert sampled.tobytes() == R.prefilter_level(chain, 4, api.lobe_sample_table(api.LOBE_LAMBERT, 1.0, 256, n, 5)).tobytes()
    assert t.mip_level_count() == 1                        # the source is left as it was
    assert irr.convert(Format.BC6H, Type.UFloat)
    result, data = irr.save_bytes(FileType.DDS)
    assert result == SaveResult.Success
    back = Texture.load(data, FileType.DDS)
    assert back is not None and back.dimension() == Dimension.Cube and back.format() == Format.BC6H and back.width(0) == 4
    # a sheen chain in place; a level so sharp that none of its records stays above the horizon is refused
    assert t.prefilter_lobe(api.LOBE_CHARLIE, mip_levels=3, samples=256, roughness=[0.0, 0.2, 1.0]) is False
    assert t.mip_level_count() == 1
    assert t.prefilter_lobe(api.LOBE_CHARLIE, mip_levels=3, samples=64, roughness=[0.0, 0.5, 1.0]) and t.mip_level_count() == 3
    tables = [None] + [api.lobe_sample_table(api.LOBE_CHARLIE, r, 64, n, 5) for r in (0.5, 1.0)]
    want = R.prefilter(chain, tables)
    for k in range(3):
        level = np.stack([t.get_image(CubeFace(f), k) for f in range(6)])
        assert same_bytes_or_both_nan(level, want[k]) and np.isfinite(level).all(), k
