"""The twin of the lobe tables, the BRDF lookup table and the irradiance cube (tests/envlobe_ref.py) against what it must
mean, without a GPU: the tables' laws, the Lambert level against the nine coefficients on an environment they represent
exactly, the lookup table against a quadrature that shares nothing with it but the BRDF, and the irradiance cube against
api.sh9_irradiance bit for bit."""
import functools

import numpy as np
import pytest

import envlobe_ref as E
import envmap_ref as R

KINDS = (E.LOBE_GGX, E.LOBE_CHARLIE, E.LOBE_LAMBERT)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("roughness", [0.3, 0.5, 1.0])
def test_table_laws(kind, roughness):
    for samples, n, levels in ((64, 16, 5), (1088, 256, 9), (4096, 5, 1)):
        t = E.lobe_sample_table(kind, roughness, samples, n, levels)
        assert t.shape == (samples, 4) and t.dtype == np.float32 and np.isfinite(t).all()      # S stays fixed
        lx, ly, lz, lod = (t[:, c].astype(np.float64) for c in range(4))
        assert (lz >= 0).all() and (lod >= 0).all() and (lod <= levels - 1).all()
        up = lz > 0
        assert up.any() and np.abs(np.sqrt(lx*lx + ly*ly + lz*lz)[up] - 1.0).max() < 4e-7      # float32 components
        assert (lod[~up] == 0).all()
        if kind == E.LOBE_GGX:
            assert t.tobytes() == R.ggx_sample_table(roughness, samples, n, levels).tobytes()
        if kind == E.LOBE_LAMBERT:
            assert up.all() and np.unique(lod).size == 1                                       # a constant density
            assert t.tobytes() == E.lobe_sample_table(kind, 0.123, samples, n, levels).tobytes()   # roughness is not read
            # uniform in the cosine: the weights' mean is the hemisphere's mean cosine
            assert abs(lz.mean() - 0.5) < 1e-6


def test_a_sharp_charlie_lobe_keeps_few_records():
    """the sheen distribution peaks at grazing half vectors, and a reflection about those points below the horizon: only
    xi1 < 2^-((2 alpha + 1) / (2 alpha)) survives, at roughness 0.25 one record in 512 -- S stays fixed, the
    weights say so, and the Python conveniences refuse a level that no record is left for"""
    for roughness, samples in ((0.25, 256), (0.25, 4096), (0.5, 256), (1.0, 64)):
        t = E.lobe_sample_table(E.LOBE_CHARLIE, roughness, samples, 16, 5)
        a = roughness*roughness
        assert abs(int((t[:, 2] > 0).sum()) - samples*2.0**(-(2.0*a + 1.0)/(2.0*a))) <= 1.0
    assert not E.lobe_sample_table(E.LOBE_CHARLIE, 0.2, 256, 16, 5)[:, 2].any()


def test_tables_refuse_what_has_no_table():
    for bad in (dict(kind=3), dict(kind=-1), dict(samples=100), dict(samples=32), dict(samples=8192), dict(face_size=0),
                dict(source_levels=6), dict(kind=E.LOBE_CHARLIE, roughness=0.0), dict(kind=E.LOBE_CHARLIE, roughness=1.5)):
        with pytest.raises(ValueError):
            E.lobe_sample_table(**dict(dict(kind=E.LOBE_LAMBERT, roughness=0.5, samples=64, face_size=16, source_levels=5), **bad))
    for samples in (0, 32, 100, 8192):
        with pytest.raises(ValueError):
            E.hammersley_table(samples)
    h = E.hammersley_table(192)
    assert h.shape == (192, 4) and (h[:, 3] == 0).all() and (h[:, 2] > 0).all() and (h[:, 2] < 1).all()
    assert np.abs(h[:, 0].astype(np.float64)**2 + h[:, 1].astype(np.float64)**2 - 1.0).max() < 2e-7


def quadratic_environment(n):
    """a polynomial of degree <= 2 in the direction, positive, different per channel -> (6, n, n, 4) float32"""
    x, y, z = R.texel_normals(n)
    c = [1.0 + 0.5*x - 0.3*y + 0.2*z + 0.4*x*y - 0.25*y*z + 0.3*(3.0*z*z - 1.0),
         0.8 - 0.4*z + 0.35*x*z + 0.2*(x*x - y*y),
         0.6 + 0.3*y + 0.1*x*y,
         np.ones_like(x)]
    return np.stack(c, -1).astype(np.float32)


def box_chain(faces):
    """the Box chain of a power-of-two cube: every level the mean of 2 x 2 texels, in double, rounded to float"""
    chain = [faces]
    while chain[-1].shape[1] > 1:
        a = chain[-1].astype(np.float64)
        chain.append(((a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2])/4.0).astype(np.float32))
    return chain


def test_lambert_level_is_the_sh9_irradiance_over_pi():
    """an environment of degree <= 2 has no band above the third: nine coefficients give its irradiance exactly, and the
    Lambert level -- uniform directions weighted by the cosine -- must estimate the same number"""
    from cuttlefish_amd import api
    n, m, S = 32, 8, 4096
    faces = quadratic_environment(n)
    chain = box_chain(faces)
    table = E.lobe_sample_table(E.LOBE_LAMBERT, 1.0, S, n, len(chain))
    got = R.prefilter_level(chain, m, table).astype(np.float64)
    coeffs = R.sh9(faces)[:36].reshape(9, 4)
    want = api.sh9_irradiance(coeffs, np.stack(R.texel_normals(m), -1))/np.pi
    worst = float(np.abs(got - want).max())
    print("Lambert level %d^2 of a %d^2 cube, S = %d: largest difference from sh9_irradiance / pi %.3g" % (m, n, S, worst))
    # measured here: 1.36e-3 (of values between 0.3 and 1.6); twice that covers Hammersley error at other phases
    assert worst <= 2.0*1.36e-3
    assert np.abs(got[..., 3] - 1.0).max() < 1e-6          # a constant channel stays


LUT_N = 6                                                  # N.V and roughness at (k + 0.5) / 6


@functools.lru_cache(maxsize=None)
def lut_and_quadrature():
    """the twin's table at S = 4096, once, and the quadrature at the same texels where the grid resolves the lobe"""
    lut = E.brdf_lut(LUT_N, LUT_N, E.hammersley_table(4096), sheen=True).astype(np.float64)
    quad = np.full((LUT_N, LUT_N, 3), np.nan)
    for y in range(LUT_N):
        for x in range(LUT_N):
            r = (y + 0.5)/LUT_N
            if r >= 0.2:
                quad[y, x] = E.brdf_quadrature((x + 0.5)/LUT_N, r)
    return lut, quad


# measured here at S = 4096 against the 512 x 1024 grid: 5.19e-3 for A and B (r >= 0.3; the largest at the most grazing
# N.V, where the grid's and the sampler's errors are both largest) and 5.4e-5 for C (r >= 0.2); twice each
GGX_MARGIN = 2.0*5.19e-3
CHARLIE_MARGIN = 2.0*5.4e-5


def test_lookup_table_against_independent_quadrature():
    lut, quad = lut_and_quadrature()
    r = (np.arange(LUT_N) + 0.5)/LUT_N
    ggx = np.abs(lut[r >= 0.3, :, :2] - quad[r >= 0.3, :, :2])
    charlie = np.abs(lut[r >= 0.2, :, 2] - quad[r >= 0.2, :, 2])
    print("lookup table against quadrature: GGX %.3g, Charlie %.3g" % (ggx.max(), charlie.max()))
    assert ggx.max() <= GGX_MARGIN and charlie.max() <= CHARLIE_MARGIN


def test_lookup_table_laws():
    lut, _ = lut_and_quadrature()
    A, B, C = lut[..., 0], lut[..., 1], lut[..., 2]
    assert (A >= 0).all() and (B >= 0).all() and (C >= 0).all() and (lut[..., 3] == 1.0).all()
    assert (A + B <= 1.0 + GGX_MARGIN).all()
    # facing the surface, a rougher one reflects less into the upper hemisphere; a smooth one loses nothing
    head_on = (A + B)[:, -1]
    assert (np.diff(head_on) < 0).all() and abs(head_on[0] - 1.0) <= GGX_MARGIN
    # without sheen the third channel is exactly 0 and the first two are the same bits
    plain = E.brdf_lut(LUT_N, LUT_N, E.hammersley_table(4096), sheen=False)
    assert (plain[..., 2] == 0).all() and plain[..., :2].tobytes() == lut[..., :2].astype(np.float32).tobytes()


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_irradiance_cube_is_sh9_irradiance_at_the_texels_bit_for_bit(n):
    from cuttlefish_amd import api
    rng = np.random.default_rng(n)
    record = np.concatenate([rng.standard_normal(36), [4.0*np.pi]])
    d = np.stack(R.texel_normals(n), -1)
    want = api.sh9_irradiance(record[:36].reshape(9, 4), d)
    assert E.cube_irradiance(record, n).tobytes() == want.astype(np.float32).tobytes()
    assert E.cube_irradiance(record, n, over_pi=True).tobytes() == (want/R.PI).astype(np.float32).tobytes()
    assert E.cube_irradiance(record, n).shape == (6, n, n, 4)
