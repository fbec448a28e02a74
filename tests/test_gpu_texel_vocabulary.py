"""The passes that decode a component all decode it the way csrc/cf_texel.h says: one small surface per pixel type whose
texels enumerate the values of a component, through alpha coverage, alpha bleeding, the signed distance field, height
ambient occlusion (every destination type, so the shared store is hit too), specular anti-aliasing and the panorama pass,
each against its own numpy twin to the exactness of that pass's own GPU test -- bit for bit, but for the panorama, whose
bound is test_gpu_envmap.py's.  Most passes quantise or threshold what they decode; the coverage count with a threshold
at a byte's decoded value and at the next float above it pins the device's table to the bit for a handful of bytes.

The surfaces (all four components of a texel hold the texel's value, so whichever component a pass reads enumerates them):
  RGBA8    64 x 4: all 256 values
  RGBA16F  64 x 4: 256 halves -- +-0, the smallest and largest subnormal, the smallest normal, the three around 1, 65504,
           +-inf, two NaNs with different payloads, seeded random finite bit patterns for the rest
  RGBA32F  64 x 5: the float images of those halves, and a fifth row of 64 floats that no half represents (among them the
           largest float, the smallest subnormal, 1 + 2^-23, 65520 and seeded random finite bit patterns)
The four values that are not finite sit in column 0, so that in the panorama pass, which blends two columns and two rows,
every other value also reaches texels whose result is finite.  That pass reads a quarter of the longitudes on face 4: the
surface is rolled by 16 columns four times, and the taps the definition reads are checked to cover every texel.

No value is excluded: every twin defines every value here (a NaN alpha is no seed, outside, and never counted; a height
that is not finite reads 0; a normal whose length is not finite is +z; NaN and infinity pass through the panorama's IEEE
arithmetic, where the comparison asks for the twin's NaN or the twin's infinity)."""
import numpy as np
import pytest

import alpha_bleed_ref
import alpha_sdf_ref
import envmap_ref
import height_ao_ref
import mip_post_ref
import spec_aa_ref
from cuttlefish_amd import api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)
W = 64
SPECIAL_HALVES = (0x7C00, 0xFC00, 0x7E01, 0xFF55,                  # +-inf and two NaNs: column 0
                  0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x3BFF, 0x3C00, 0x3C01, 0x7BFF)
# (t, scale): t is in (0, 1]; the scales bring the large values of the float surfaces down to it
COVERAGE = ((2.0**-24, 1.0), (0.25, 1.0), (0.5, 1.0), (0.5, 1.75), (1.0, 1.0), (1.0, 2.0**-10), (1.0, 2.0**-16), (2.0**-14, 4.0))
# ... and the decode of a byte to the bit: a threshold at (float)(v / 255.0) counts the 256 - v bytes from v up, the next
# float above it one fewer, so a table entry one ulp off moves a count
PINNED_BYTES = (1, 2, 3, 85, 127, 128, 170, 253, 254)
_PINS = [np.float32(v/255.0) for v in PINNED_BYTES]
COVERAGE += tuple((float(t), 1.0) for f in _PINS for t in (f, np.nextafter(f, np.float32(2.0))))
FACE, FACE_SIZE, ROLLS = 4, 32, (0, 16, 32, 48)
_SURFACES = {}


def _halves():
    rng = np.random.default_rng(2024)
    rest = []
    while len(rest) < 256 - len(SPECIAL_HALVES):
        b = int(rng.integers(0, 65536))
        if (b & 0x7C00) != 0x7C00 and b not in SPECIAL_HALVES and b not in rest:
            rest.append(b)
    return np.array(SPECIAL_HALVES + tuple(rest), np.uint16).view(np.float16)


def _floats_no_half_holds():
    rng = np.random.default_rng(2025)
    fixed = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 2.0**-149, 1.0 + 2.0**-23, 65520.0, 2.0**-25,
                      -2.0**-25, 1.0/3.0], np.float32)
    rest = []
    while len(rest) < W - fixed.size:
        f = np.array([rng.integers(0, 2**32)], np.uint32).view(np.float32)[0]
        with np.errstate(over="ignore"):
            if np.isfinite(f) and np.float32(np.float16(f)) != f:
                rest.append(f)
    out = np.concatenate([fixed, np.array(rest, np.float32)])
    with np.errstate(over="ignore"):
        assert (out.astype(np.float16).astype(np.float32) != out).all()
    return out


def surface(dtype):
    """(rows, 64, 4): value i of the enumeration in all four components of its texel, the first four values in column 0"""
    dtype = np.dtype(dtype)
    if dtype not in _SURFACES:
        if dtype == np.uint8:
            v = np.arange(256, dtype=np.uint8)
        else:
            v = _halves()
            if dtype == np.float32:
                v = np.concatenate([v.astype(np.float32), _floats_no_half_holds()])
            # the four that are not finite to texels (0, 0) ... (0, 3): swapped with what was there
            for j in range(1, 4):
                v[[j, j*W]] = v[[j*W, j]]
            assert not np.isfinite(v.reshape(-1, W)[:4, 0]).any() and np.isfinite(v.reshape(-1, W)[:, 1:]).all()
        _SURFACES[dtype] = np.repeat(v.reshape(-1, W)[:, :, None], 4, axis=2)
    return _SURFACES[dtype]


def panorama_taps(width, height, n):
    """the (row, column) pairs the definition reads for face 4 at supersample 1 (envmap_ref.equirect_to_cube's steps)"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    dx, dy, dz = envmap_ref.face_dir(np.full(x.shape, FACE), envmap_ref.centre(x, n), envmap_ref.centre(y, n))
    phi, psi = np.arctan2(dx, dz), np.arcsin(dy/np.sqrt((dx*dx + dy*dy) + dz*dz))
    x0 = np.floor((phi/(2.0*envmap_ref.PI) + 0.5)*float(width) - 0.5).astype(np.int64)
    y0 = np.floor((0.5 - psi/envmap_ref.PI)*float(height) - 0.5).astype(np.int64)
    xs = ((x0 % width).ravel(), ((x0 + 1) % width).ravel())
    ys = (np.clip(y0, 0, height - 1).ravel(), np.clip(y0 + 1, 0, height - 1).ravel())
    return {(int(r), int(c)) for rows in ys for cols in xs for r, c in zip(rows, cols)}


def twins(img, ao_table):
    """what the six twins make of a surface; every one of them has to accept every value of it"""
    out = {}
    out["coverage"] = [mip_post_ref.coverage(img, np.float32(t), np.float32(s)) for t, s in COVERAGE]
    out["bleed"] = alpha_bleed_ref.bleed(img, 0.25)
    out["sdf"] = alpha_sdf_ref.sdf(img, 1)
    for dst in DTYPES:
        for mask, channels in ((1, "r"), (15, "rgba")):
            into = np.array(img) if img.dtype == dst else np.zeros(img.shape, dst)
            out["ao", np.dtype(dst).name, channels] = height_ao_ref.height_ao(img, into, 1, D=8, channel=2, mask=mask,
                                                                              table=ao_table)
    out["spec_aa"] = spec_aa_ref.specular_aa(img, img, 2, channel=1)
    out["cube"] = [envmap_ref.equirect_to_cube(np.roll(img, r, axis=1), FACE_SIZE, 1) for r in ROLLS]
    return out


@pytest.fixture(scope="module", params=DTYPES, ids=lambda d: np.dtype(d).name)
def case(request):
    img = surface(request.param)
    return img, twins(img, api.height_ao_directions(8))


def test_alpha_coverage_counts(gpu_ctx, case):
    img, want = case
    got = [gpu_ctx.alpha_coverage(img, t, s) for t, s in COVERAGE]
    assert got == want["coverage"]
    if img.dtype == np.uint8:
        assert got[-2*len(PINNED_BYTES):] == [256 - v - up for v in PINNED_BYTES for up in (0, 1)]


def test_alpha_bleed_seeds(gpu_ctx, case):
    img, (want, wrec) = case[0], case[1]["bleed"]
    got, rec = gpu_ctx.alpha_bleed(img, 0.25)
    assert rec["seeds"] == wrec["seeds"] and rec == wrec
    assert got.tobytes() == want.tobytes()


def test_alpha_sdf_inside(gpu_ctx, case):
    img, (want, wrec) = case[0], case[1]["sdf"]
    got, rec = gpu_ctx.alpha_sdf(img, 1)
    assert rec["inside"] == wrec["inside"] and rec == wrec
    assert got.tobytes() == alpha_sdf_ref.apply(img, want).tobytes()


@pytest.mark.parametrize("channels", ["r", "rgba"])
@pytest.mark.parametrize("dst", DTYPES, ids=lambda d: np.dtype(d).name)
def test_height_ao_reads_and_stores(gpu_ctx, case, dst, channels):
    img, (want, wrec) = case[0], case[1]["ao", np.dtype(dst).name, channels]
    got, rec = gpu_ctx.height_ao(img, 1, directions=8, channel="b", channels=channels, out_dtype=dst)
    assert got.tobytes() == want.tobytes() and rec == wrec


def test_specular_aa_normals_and_roughness(gpu_ctx, case):
    img, (want, wrec) = case[0], case[1]["spec_aa"]
    got, rec = gpu_ctx.specular_aa(img, img, 2, channel="g")
    assert len(got) == 1 and got[0].tobytes() == want[0].tobytes() and rec == wrec


def test_panorama_to_cube(gpu_ctx, case):
    img, want = case[0], case[1]["cube"]
    h = img.shape[0]
    read = set()
    for roll, (faces, spread) in zip(ROLLS, want):
        got = gpu_ctx.equirect_to_cube(np.roll(img, roll, axis=1), FACE_SIZE, supersample=1)[FACE].astype(np.float64)
        ref, spread = faces[FACE].astype(np.float64), spread[FACE]
        finite = np.isfinite(ref)
        # the twin's NaN is a NaN, the twin's infinity that infinity
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
        assert np.isfinite(spread[finite]).all()
        # test_gpu_envmap.py's bound: atan2 and asin are the device library's
        bound = np.spacing(np.abs(ref[finite]).astype(np.float32)).astype(np.float64) + 2.0*2.0**-40*max(W, h)*spread[finite]
        assert (np.abs(got[finite] - ref[finite]) <= bound).all(), roll
        read |= {(r, (c - roll) % W) for r, c in panorama_taps(W, h, FACE_SIZE)}
    assert read == {(r, c) for r in range(h) for c in range(W)}
