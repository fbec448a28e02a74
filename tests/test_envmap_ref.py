"""The numpy twin of the environment-map entries (tests/envmap_ref.py) against independent facts: the face table and its
inverse, the seamless tap against a search over all texels, panoramas with known answers, the sample table's laws, the
lobe's peak, and the nine coefficients against plain quadrature.  No GPU."""
import numpy as np
import pytest

import envmap_ref as R


def all_normals(n):
    """(6 n n, 3): the unit directions of every texel centre, in (face, y, x) order"""
    return np.stack([v.reshape(-1) for v in R.texel_normals(n)], -1)


def box_chain(faces):
    """a full chain by 2 x 2 means in float32: an input for the lobe, nothing more"""
    chain = [np.asarray(faces, np.float32)]
    while chain[-1].shape[1] > 1:
        a = chain[-1]
        m = a.shape[1]//2
        a = a[:, :2*m, :2*m]
        chain.append(((a[:, 0::2, 0::2] + a[:, 1::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 1::2])*np.float32(0.25)))
    return chain


def paint(function, W, H):
    """an equirectangular panorama of a function of direction, sampled at the pixel centres, as float64 (H, W)"""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    phi = ((i + 0.5)/W - 0.5)*2.0*np.pi
    psi = (0.5 - (j + 0.5)/H)*np.pi
    return function(np.sin(phi)*np.cos(psi), np.sin(psi), np.cos(phi)*np.cos(psi))


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_direction_and_face_round_trip_is_exact_at_texel_centres(n):
    f, y, x = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    s, t = R.centre(x, n), R.centre(y, n)
    dx, dy, dz = R.face_dir(f, s, t)
    f2, s2, t2 = R.dir_to_face(dx, dy, dz)
    assert (f2 == f).all() and (s2 == s).all() and (t2 == t).all()
    # and of the normalised direction: the same face, (s, t) within rounding
    f3, s3, t3 = R.dir_to_face(*R.normalise(dx, dy, dz))
    assert (f3 == f).all() and np.abs(s3 - s).max() < 1e-15 and np.abs(t3 - t).max() < 1e-15
    # the six face centres look along the six axes, +Y up
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for face, axis in enumerate(axes):
        assert tuple(float(v) for v in R.face_dir(face, 0.0, 0.0)) == axis
    assert float(R.face_dir(4, 0.0, -0.5)[1]) == 0.5               # y downward: t < 0 looks up


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_an_off_face_tap_is_the_texel_a_search_over_all_directions_finds(n):
    """every tap of the ring around every face: the texel it resolves to is the one whose direction is nearest the tap's
    -- the largest dot product over all 6 n^2 texels, ties (the cube's corners) included"""
    normals = all_normals(n)
    ring = [(i, j) for i in range(-1, n + 1) for j in range(-1, n + 1) if not (0 <= i < n and 0 <= j < n)]
    for f in range(6):
        i, j = np.array(ring).T
        ff, ii, jj = R.resolve_tap(np.full(i.shape, f), i, j, n)
        d = np.stack(R.normalise(*R.face_dir(np.full(i.shape, f), R.centre(i.astype(float), n), R.centre(j.astype(float), n))), -1)
        dots = d @ normals.T                                        # (taps, texels)
        got = dots[np.arange(len(ring)), (ff*n + jj)*n + ii]
        assert (got >= dots.max(1) - 1e-12).all(), (n, f)
        assert (ff != f).all()                                      # never the face it left
    # inside taps are themselves
    ff, ii, jj = R.resolve_tap(np.array([3]), np.array([n - 1]), np.array([0]), n)
    assert (int(ff[0]), int(ii[0]), int(jj[0])) == (3, n - 1, 0)


def test_fetch_at_a_texel_centre_is_the_texel_and_across_an_edge_is_continuous():
    rng = np.random.default_rng(1)
    faces = rng.random((6, 4, 4, 4)).astype(np.float32)
    f, y, x = np.meshgrid(np.arange(6), np.arange(4), np.arange(4), indexing="ij")
    got = R.fetch(faces, f, R.centre(x, 4), R.centre(y, 4))
    assert (got == faces.astype(np.float64)).all()
    # the same direction reached from +Z's right edge and from +X's left edge: s = 1 on +Z is s = -1 on +X (away from
    # the corners, where the taps beyond two edges are replaced from different planes)
    t = np.linspace(-0.7, 0.7, 7)
    a = R.fetch(faces, np.full(7, 4), np.full(7, 1.0), t)
    b = R.fetch(faces, np.full(7, 0), np.full(7, -1.0), t)
    assert np.abs(a - b).max() < 1e-15


def test_sum64_is_the_lane_sums_then_the_butterfly():
    rng = np.random.default_rng(2)
    v = rng.standard_normal(192)*10.0**rng.integers(-8, 8, 192)
    p = [0.0]*64
    for i, x in enumerate(v):
        p[i % 64] = p[i % 64] + x
    for m in (32, 16, 8, 4, 2, 1):
        p = [p[j] + p[j ^ m] for j in range(64)]
    assert float(R.sum64(v)) == p[0] and len(set(p)) == 1


@pytest.mark.parametrize("dtype,value", [(np.float32, 0.1), (np.float16, 0.3), (np.uint8, 77), (np.float32, 12345.678)])
def test_a_constant_panorama_gives_constant_faces_bit_for_bit(dtype, value):
    pano = np.full((5, 9, 4), value, dtype)
    for n, q in ((1, 1), (3, 2), (8, 4)):
        faces, spread = R.equirect_to_cube(pano, n, q)
        assert faces.dtype == np.float32 and faces.shape == (6, n, n, 4)
        assert (faces == R.to_float(pano)[0, 0, 0]).all() and (spread == 0).all()


def test_a_smooth_panorama_reproduces_its_function_within_the_bilinear_error():
    """a low-order function of direction painted at 128 x 64 and read back at the texel centres of 8^2 faces with one
    sample per texel.  No texel of an even face size lies within half a panorama row of a pole (asserted through R: no
    tap was clamped), so the error is that of bilinear interpolation: at most (Mxx + Myy) / 8, M the largest second
    differences of the painted grid along x (wrapped) and y -- interpolating along x errs by at most Mxx / 8 in either
    row, the blend of the two rows along y by Myy / 8.  A second difference of the grid is h^2 f'' at a nearby point, not
    at the worst one: 10 % is allowed for that, and a float32 rounding of the painted values and of the result."""
    def function(x, y, z):
        return 0.5 + 0.3*x - 0.2*y*z + 0.25*z*z + 0.1*x*y

    W, H, n = 128, 64, 8
    grid = paint(function, W, H)
    pano = np.repeat(grid[..., None], 4, -1).astype(np.float32)
    faces, _ = R.equirect_to_cube(pano, n, 1)
    nx, ny, nz = R.texel_normals(n)
    assert (np.abs(np.arcsin(ny)) < np.pi/2 - np.pi/H).all()        # a row and a half from the poles: nothing clamped
    mxx = np.abs(np.roll(grid, 1, 1) - 2.0*grid + np.roll(grid, -1, 1)).max()
    myy = np.abs(grid[:-2] - 2.0*grid[1:-1] + grid[2:]).max()
    bound = 1.1*(mxx + myy)/8.0 + 3.0*2.0**-24
    err = np.abs(faces[..., 0].astype(np.float64) - function(nx, ny, nz)).max()
    print("bilinear error %.3g, bound %.3g" % (err, bound))
    assert 0 < err <= bound and (faces[..., 0] == faces[..., 3]).all()
    # orientation: +X of the cube is the panorama's right quarter, +Y its top
    marks = paint(lambda x, y, z: (x > 0.9)*1.0 + (y > 0.9)*2.0 + (z > 0.9)*4.0, W, H)
    faces, _ = R.equirect_to_cube(np.repeat(marks[..., None], 4, -1).astype(np.float32), 3, 1)
    assert [float(faces[f, 1, 1, 0]) for f in range(6)] == [1.0, 0.0, 2.0, 0.0, 4.0, 0.0]


def test_supersampling_is_the_mean_of_its_sub_samples():
    rng = np.random.default_rng(3)
    pano = rng.random((16, 32, 4)).astype(np.float32)
    fine, _ = R.equirect_to_cube(pano, 8, 1)
    coarse, _ = R.equirect_to_cube(pano, 4, 2)
    mean = (fine[:, 0::2, 0::2].astype(np.float64) + fine[:, 0::2, 1::2] + fine[:, 1::2, 0::2] + fine[:, 1::2, 1::2])/4.0
    assert np.abs(coarse - mean).max() < 1e-6


@pytest.mark.parametrize("roughness", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("samples", [64, 1024])
def test_sample_table_laws(roughness, samples):
    levels = 6
    t = R.ggx_sample_table(roughness, samples, 32, levels).astype(np.float64)
    assert t.shape == (samples, 4)
    lx, ly, lz, lod = t.T
    above = lz > 0
    assert above.any() and (lz >= 0).all()
    assert np.abs(np.sqrt(lx*lx + ly*ly + lz*lz)[above] - 1.0).max() <= 2.0**-22
    assert ((lx*lx + ly*ly)[~above] <= 1.0 + 2.0**-22).all() and (lod[~above] == 0).all()
    assert (lod >= 0).all() and (lod <= levels - 1).all()
    # the density falls with the sample index (xi1 rises, the half vector tilts away): the level may not fall with it
    assert (np.diff(lod[above]) >= 0).all()
    if roughness == 1.0:
        assert not above.all()                                     # some reflections leave the hemisphere


def test_sample_table_refuses_what_has_no_table():
    for bad in (dict(roughness=0.0), dict(roughness=-0.5), dict(roughness=1.5), dict(roughness=float("nan")),
                dict(samples=0), dict(samples=32), dict(samples=100), dict(samples=8192),
                dict(face_size=0), dict(source_levels=0), dict(source_levels=7)):
        with pytest.raises(ValueError):
            R.ggx_sample_table(**dict(dict(roughness=0.5, samples=64, face_size=32, source_levels=6), **bad))


def test_the_peak_of_one_bright_texel_stays_put_and_falls_as_roughness_rises():
    n = 8
    faces = np.zeros((6, n, n, 4), np.float32)
    faces[4, 2, 5] = 1000.0
    chain = box_chain(faces)
    peaks = []
    for r in (0.2, 0.5, 1.0):
        out = R.prefilter_level(chain, n, R.ggx_sample_table(r, 256, n, len(chain)))
        assert np.unravel_index(np.argmax(out[..., 0]), out.shape[:3]) == (4, 2, 5), r
        assert (out >= 0).all() and (out[..., 0] == out[..., 3]).all()
        peaks.append(float(out[4, 2, 5, 0]))
    print("peaks", peaks)
    assert 1000.0 > peaks[0] > peaks[1] > peaks[2] > 0
    # a constant environment stays constant under any lobe, at any level
    flat = box_chain(np.full((6, n, n, 4), 0.375, np.float32))
    for size in (8, 2, 1):
        assert (R.prefilter_level(flat, size, R.ggx_sample_table(0.6, 64, n, len(flat))) == np.float32(0.375)).all()
    # roughness 0 is the source level itself
    assert R.prefilter(chain, [None, None])[1].tobytes() == chain[1].tobytes()


def test_sh9_of_a_constant_environment():
    for n in (1, 3, 16, 65):
        c = np.array([0.25, 1.0, 3.5, 0.0])
        out = R.sh9(np.broadcast_to(c.astype(np.float32), (6, n, n, 4)))
        want = np.zeros((9, 4))
        want[0] = np.sqrt(4.0*np.pi)*c
        assert np.abs(out[:36].reshape(9, 4) - want).max() <= 1e-12, n
        # the texels' solid angles are those of the sphere, the better the finer the faces
        assert abs(out[36] - 4.0*np.pi) <= 4.0*np.pi/(n*n) + 1e-12


@pytest.mark.parametrize("n", [16, 33])
def test_sh9_of_one_basis_function_against_plain_quadrature(n):
    nx, ny, nz = R.texel_normals(n)
    basis = R.sh_basis(nx, ny, nz)
    dw = np.broadcast_to(R.solid_angles(n), (6, n, n))
    for b in range(9):
        faces = np.repeat(basis[b][..., None], 4, -1).astype(np.float32)
        got = R.sh9(faces)[:36].reshape(9, 4)
        # the same sums in float64 from numpy's own summation: the arithmetic is the same, the order is not
        c = faces[..., 0].astype(np.float64)
        brute = np.array([np.sum(c*(basis[k]*dw)) for k in range(9)])*(4.0*np.pi/np.sum(dw))
        assert np.abs(got[:, 0] - brute).max() <= 1e-12 and (got[:, 0:1] == got).all()
        others = np.delete(got[:, 0], b)
        assert abs(got[b, 0] - 1.0) < 0.02 and np.abs(others).max() < 0.02, (b, got[:, 0])


def test_sh9_irradiance_of_a_constant_environment_is_pi_times_it():
    coeffs = R.sh9(np.full((6, 8, 8, 4), 2.0, np.float32))[:36].reshape(9, 4)
    d = all_normals(3)
    assert np.abs(R.sh9_irradiance(coeffs, d) - 2.0*np.pi).max() < 1e-11
