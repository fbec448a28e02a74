"""numpy twin of the environment-map entries (include/cuttlefish_hip.h: cfhip_equirect_to_cube_device,
cfhip_cube_prefilter_device, cfhip_cube_sh9_device, cfhip_ggx_sample_table), written from the
definition alone.  Every formula is a sequence of IEEE double operations in the order the header states, so the kernels
return this file's bits -- except for part 1's atan2 / asin and the table helper's cos / sin / log2, which come from
different math libraries.  The twin is the definition.

Faces are in CubeFace order (+X, -X, +Y, -Y, +Z, -Z); a face set is a (6, n, n, 4) float32 array, a chain a list of them."""
import numpy as np

PI = 3.141592653589793
MAX_FACE = 8192
MAX_PANORAMA = 32768
SUPERSAMPLES = (1, 2, 4)
MIN_SAMPLES, MAX_SAMPLES = 64, 4096
# the real spherical-harmonic basis: the constants the header quotes to six places, in full
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = 1.0925484305920792
SH_C20 = 0.31539156525252005
SH_C22 = 0.5462742152960396


def to_float(image: np.ndarray) -> np.ndarray:
    """texels as float32: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored"""
    a = np.asarray(image)
    if a.dtype == np.uint8:
        return (a.astype(np.float64)/255.0).astype(np.float32)
    if a.dtype in (np.float16, np.float32):
        return a.astype(np.float32)
    raise TypeError("pixel dtype %s" % a.dtype)


def centre(i, n, a=0.5):
    """s (or t) of position i + a on a face of size n"""
    return (2.0*(i + a))/float(n) - 1.0


def face_dir(f, s, t):
    """the direction d(f, s, t) of the face table, not normalised"""
    f = np.asarray(f)
    s = np.asarray(s, np.float64)
    t = np.asarray(t, np.float64)
    one = np.ones(np.broadcast(f, s, t).shape)
    x = np.choose(f, [one, -one, s*one, s*one, s*one, -s*one])
    y = np.choose(f, [-t*one, -t*one, one, -one, -t*one, -t*one])
    z = np.choose(f, [-s*one, s*one, t*one, -t*one, one, -one])
    return x, y, z


def normalise(x, y, z):
    r = np.sqrt((x*x + y*y) + z*z)
    return x/r, y/r, z/r


def dir_to_face(x, y, z):
    """-> (face, s, t): the major axis is X if |x| >= |y| and |x| >= |z|, else Y if |y| >= |z|, else Z; its sign picks the
    face (negative: the odd one); (s, t) invert the face table, divided by the major component's magnitude"""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(invalid="ignore", divide="ignore"):
        isx = (ax >= ay) & (ax >= az)
        isy = ~isx & (ay >= az)
        f = np.where(isx, np.where(x < 0, 1, 0), np.where(isy, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
        ma = np.where(isx, ax, np.where(isy, ay, az))
        s = np.choose(f, [-z, z, x, x, x, -x])/ma
        t = np.choose(f, [-y, -y, z, -z, -y, -y])/ma
    return f, s, t


def _floor_index(p, lo, hi):
    """floor(p) held to [lo, hi] as float64; a NaN becomes lo"""
    with np.errstate(invalid="ignore"):
        q = np.floor(p)
        q = np.where(q >= lo, q, float(lo))
        return np.where(q > hi, float(hi), q)


def resolve_tap(f, i, j, n):
    """the texel (face, x, y) that tap (i, j) of face f stands for: itself inside [0, n)^2; outside, its centre on the
    extended face plane becomes a direction, the face is selected again and the nearest texel there is taken"""
    f, i, j = np.broadcast_arrays(np.asarray(f), np.asarray(i), np.asarray(j))
    inside = (i >= 0) & (i < n) & (j >= 0) & (j < n)
    x, y, z = face_dir(f, centre(i.astype(np.float64), n), centre(j.astype(np.float64), n))
    f2, s2, t2 = dir_to_face(x, y, z)
    i2 = _floor_index(((s2 + 1.0)*0.5)*float(n), 0, n - 1).astype(np.int64)
    j2 = _floor_index(((t2 + 1.0)*0.5)*float(n), 0, n - 1).astype(np.int64)
    return np.where(inside, f, f2), np.where(inside, i, i2), np.where(inside, j, j2)


def fetch(faces: np.ndarray, f, s, t) -> np.ndarray:
    """the seamless bilinear fetch of (face, s, t) from a (6, n, n, 4) face set -> (..., 4) float64"""
    n = faces.shape[1]
    s = np.asarray(s, np.float64)
    t = np.asarray(t, np.float64)
    px = ((s + 1.0)*0.5)*float(n) - 0.5
    py = ((t + 1.0)*0.5)*float(n) - 0.5
    x0 = _floor_index(px, -1, n - 1)
    y0 = _floor_index(py, -1, n - 1)
    fx = (px - x0)[..., None]
    fy = (py - y0)[..., None]
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    c = []
    for dy in (0, 1):
        for dx in (0, 1):
            ff, ii, jj = resolve_tap(f, x0 + dx, y0 + dy, n)
            c.append(faces[ff, jj, ii].astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((c[0]*(1.0 - fx) + c[1]*fx)*(1.0 - fy)) + ((c[2]*(1.0 - fx) + c[3]*fx)*fy)


def sum64(v: np.ndarray) -> np.ndarray:
    """sum64 over axis 0 (a multiple of 64 long): p_j = the sum of v_i, i = j mod 64, in increasing i from 0.0; then
    p_j += p_{j xor 32}, 16, 8, 4, 2, 1; the result is p_0"""
    v = np.asarray(v, np.float64)
    assert v.shape[0] % 64 == 0
    p = np.zeros((64,) + v.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, v.shape[0], 64):
            p = p + v[k:k + 64]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            p = p + p[lane ^ m]
    return p[0]


# ---- part 1: panorama to six faces --------------------------------------------------------------------------------------
def equirect_to_cube(panorama: np.ndarray, n: int, supersample: int = 2):
    """-> (faces (6, n, n, 4) float32, R (6, n, n, 4) float64: per texel and channel the largest minus the smallest tap
    value read)"""
    src = to_float(panorama).astype(np.float64)
    H, W = src.shape[:2]
    q = int(supersample)
    assert q in SUPERSAMPLES and 2 <= W <= MAX_PANORAMA and 1 <= H <= MAX_PANORAMA and 1 <= n <= MAX_FACE
    f, y, x = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    acc = np.zeros((6, n, n, 4))
    lo = np.full((6, n, n, 4), np.inf)
    hi = np.full((6, n, n, 4), -np.inf)
    for b in range(q):
        for a in range(q):
            dx, dy, dz = face_dir(f, centre(x, n, (a + 0.5)/q), centre(y, n, (b + 0.5)/q))
            m = (dx*dx + dy*dy) + dz*dz
            phi = np.arctan2(dx, dz)
            psi = np.arcsin(dy/np.sqrt(m))
            u = (phi/(2.0*PI) + 0.5)*float(W) - 0.5
            v = (0.5 - psi/PI)*float(H) - 0.5
            x0 = _floor_index(u, -1, W - 1)
            y0 = _floor_index(v, -1, H - 1)
            fx = (u - x0)[..., None]
            fy = (v - y0)[..., None]
            x0 = x0.astype(np.int64)
            y0 = y0.astype(np.int64)
            xa = np.where(x0 < 0, x0 + W, x0)
            xb = np.where(x0 + 1 >= W, x0 + 1 - W, x0 + 1)
            ya = np.clip(y0, 0, H - 1)
            yb = np.clip(y0 + 1, 0, H - 1)
            c00, c10, c01, c11 = src[ya, xa], src[ya, xb], src[yb, xa], src[yb, xb]
            with np.errstate(invalid="ignore", over="ignore"):
                acc = acc + (((c00*(1.0 - fx) + c10*fx)*(1.0 - fy)) + ((c01*(1.0 - fx) + c11*fx)*fy))
            for c in (c00, c10, c01, c11):
                lo = np.minimum(lo, c)
                hi = np.maximum(hi, c)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc/float(q*q)).astype(np.float32), hi - lo


# ---- part 2: the GGX chain -----------------------------------------------------------------------------------------------
def radical_inverse(i: np.ndarray) -> np.ndarray:
    """base 2: the 32 bits of i reversed, times 2^-32"""
    b = np.asarray(i, np.uint64)
    r = np.zeros_like(b)
    for k in range(32):
        r |= ((b >> np.uint64(k)) & np.uint64(1)) << np.uint64(31 - k)
    return r.astype(np.float64)*2.0**-32


def ggx_sample_table(roughness: float, samples: int, face_size: int, source_levels: int) -> np.ndarray:
    """-> (samples, 4) float32 records (lx, ly, lz, lod): Hammersley points through the GGX distribution of normals,
    reflected about (0, 0, 1); a record below the horizon keeps lx, ly and gets lz = 0, lod = 0"""
    r = float(np.float32(roughness))                       # the C helper takes a float
    S, N, L = int(samples), int(face_size), int(source_levels)
    if not (0.0 < r <= 1.0):
        raise ValueError("roughness %r outside (0, 1]" % (roughness,))
    if S % 64 or not MIN_SAMPLES <= S <= MAX_SAMPLES:
        raise ValueError("samples %r: a multiple of 64 from 64 to 4096" % (samples,))
    if not 1 <= N <= MAX_FACE or not 1 <= L <= N.bit_length():
        raise ValueError("face_size %r, source_levels %r" % (face_size, source_levels))
    i = np.arange(S)
    xi1 = (i + 0.5)/float(S)
    xi2 = radical_inverse(i)
    a = r*r
    a2 = a*a
    cos2 = (1.0 - xi1)/(1.0 + (a2 - 1.0)*xi1)
    hz = np.sqrt(cos2)
    sin = np.sqrt(1.0 - cos2)
    phi = (2.0*PI)*xi2
    hx = sin*np.cos(phi)
    hy = sin*np.sin(phi)
    lx = (2.0*hz)*hx
    ly = (2.0*hz)*hy
    lz = (2.0*hz)*hz - 1.0
    e = (hz*hz)*(a2 - 1.0) + 1.0
    pdf = (a2/(PI*(e*e)))/4.0
    lod = 0.5*np.log2((1.0/(float(S)*pdf))/((4.0*PI)/(6.0*(float(N)*float(N))))) + 1.0
    lod = np.minimum(np.maximum(lod, 0.0), float(L - 1))
    below = lz <= 0.0
    lz = np.where(below, 0.0, lz)
    lod = np.where(below, 0.0, lod)
    return np.stack([lx, ly, lz, lod], -1).astype(np.float32)


def texel_normals(n: int):
    """-> (nx, ny, nz), each (6, n, n): the normalised directions of a face set's texel centres"""
    f, y, x = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    return normalise(*face_dir(f, centre(x, n), centre(y, n)))


def prefilter_level(chain, n: int, table: np.ndarray) -> np.ndarray:
    """one destination level of size n from the source chain (a list of (6, m, m, 4) float32) and a (S, 4) float32 table
    -> (6, n, n, 4) float32"""
    L = len(chain)
    tab = np.asarray(table, np.float32).astype(np.float64)
    S = tab.shape[0]
    assert S % 64 == 0 and S >= 64
    nx, ny, nz = (v.reshape(-1) for v in texel_normals(n))
    far = np.abs(nz) < 0.999
    zero = np.zeros_like(nx)
    ax, ay, az = normalise(np.where(far, -ny, zero), np.where(far, nx, -nz), np.where(far, zero, ny))   # tx
    bx, by, bz = ny*az - nz*ay, nz*ax - nx*az, nx*ay - ny*ax                                              # ty = n x tx
    ipart = tab[:, 3].astype(np.int64)
    l0 = np.minimum(ipart, L - 1)
    l1 = np.minimum(l0 + 1, L - 1)
    g = tab[:, 3] - ipart.astype(np.float64)
    p = np.zeros((64, nx.size, 4))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(0, S, 64):
            lx, ly, lz = (tab[k:k + 64, c][:, None] for c in range(3))
            wx = (ax*lx + bx*ly) + nx*lz
            wy = (ay*lx + by*ly) + ny*lz
            wz = (az*lx + bz*ly) + nz*lz
            f, s, t = dir_to_face(wx, wy, wz)
            c = np.zeros((64, nx.size, 4))
            for j in range(64):
                a0 = fetch(chain[l0[k + j]], f[j], s[j], t[j])
                a1 = a0 if l1[k + j] == l0[k + j] else fetch(chain[l1[k + j]], f[j], s[j], t[j])
                c[j] = a0*(1.0 - g[k + j]) + a1*g[k + j]
            p = p + c*lz[..., None]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            p = p + p[lane ^ m]
        out = p[0]/sum64(tab[:, 2])
        return out.astype(np.float32).reshape(6, n, n, 4)


def prefilter(chain, tables):
    """-> the destination chain: level k from tables[k]; a table of no records copies source level k"""
    N = chain[0].shape[1]
    out = []
    for k, tab in enumerate(tables):
        if tab is None or len(tab) == 0:
            out.append(chain[k].copy())
        else:
            out.append(prefilter_level(chain, max(1, N >> k), tab))
    return out


def default_roughness(levels: int):
    return [0.0] if levels == 1 else [k/float(levels - 1) for k in range(levels)]


# ---- part 3: nine coefficients ------------------------------------------------------------------------------------------
def sh_basis(x, y, z):
    """the nine real basis values, in the order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2"""
    return [SH_C0*np.ones_like(x), SH_C1*y, SH_C1*z, SH_C1*x, SH_C2*(x*y), SH_C2*(y*z), SH_C20*(3.0*(z*z) - 1.0),
            SH_C2*(x*z), SH_C22*(x*x - y*y)]


def solid_angles(n: int) -> np.ndarray:
    """(n, n): d omega of a face's texels, (4 / n^2) / (r sqrt(r)), r = (1 + s^2) + t^2"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    s, t = centre(x, n), centre(y, n)
    r = (1.0 + s*s) + t*t
    return (4.0/(float(n)*float(n)))/(r*np.sqrt(r))


def sh9(faces: np.ndarray) -> np.ndarray:
    """-> 37 float64: coefficient b, channel c at [4 b + c], each times 4 pi / sum of d omega; then that sum.  Row
    partials are sum64 over the row padded with zeros; the rows are added in (face, y) order from 0.0"""
    faces = np.asarray(faces, np.float32)
    n = faces.shape[1]
    nx, ny, nz = texel_normals(n)
    dw = np.broadcast_to(solid_angles(n), (6, n, n))
    basis = sh_basis(nx, ny, nz)
    c = faces.astype(np.float64)
    vals = np.empty((6, n, n, 37))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(9):
            vals[..., 4*b:4*b + 4] = c*(basis[b]*dw)[..., None]
        vals[..., 36] = dw
        pad = -n % 64
        rows = np.concatenate([vals, np.zeros((6, n, pad, 37))], 2)          # (6, n, n + pad, 37)
        partial = sum64(np.moveaxis(rows, 2, 0)).reshape(6*n, 37)
        total = np.zeros(37)
        for r in range(6*n):
            total = total + partial[r]
        out = total*((4.0*PI)/total[36])
    out[36] = total[36]
    return out


def sh9_irradiance(coeffs: np.ndarray, directions: np.ndarray) -> np.ndarray:
    """the cosine-lobe convolution evaluated: coeffs (9, C), unit directions (..., 3) -> (..., C)"""
    d = np.asarray(directions, np.float64)
    k = np.asarray(coeffs, np.float64).reshape(9, -1)
    band = [PI] + [2.0*PI/3.0]*3 + [PI/4.0]*5
    basis = sh_basis(d[..., 0], d[..., 1], d[..., 2])
    return sum((band[b]*basis[b])[..., None]*k[b] for b in range(9))
