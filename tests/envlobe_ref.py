"""numpy twin of the entries that complete a split-sum shader's inputs (include/cuttlefish_hip.h: cfhip_lobe_sample_table,
cfhip_hammersley_table, cfhip_brdf_lut_device, cfhip_cube_irradiance_device), written from the
definition alone on the vocabulary of tests/envmap_ref.py.  Every formula is a sequence of IEEE double operations in the
order the header states, so the kernels return this file's bits -- except for pow of the Charlie terms and the table
helpers' cos / sin / log2, which come from different math libraries.

brdf_quadrature is no twin: it integrates the same BRDFs over a plain grid of light directions, without importance
sampling, and is what the lookup table is checked against."""
import numpy as np

import envmap_ref as R

PI = R.PI
LOBE_GGX, LOBE_CHARLIE, LOBE_LAMBERT = 0, 1, 2
MAX_LUT = 1024


def _points(samples: int):
    """the Hammersley points -> (xi1, phi)"""
    S = int(samples)
    if S % 64 or not R.MIN_SAMPLES <= S <= R.MAX_SAMPLES:
        raise ValueError("samples %r: a multiple of 64 from 64 to 4096" % (samples,))
    i = np.arange(S)
    return (i + 0.5)/float(S), (2.0*PI)*R.radical_inverse(i)


def lobe_sample_table(kind: int, roughness: float, samples: int, face_size: int, source_levels: int) -> np.ndarray:
    """-> (samples, 4) float32 records (lx, ly, lz, lod) of the lobe `kind`"""
    if kind == LOBE_GGX:
        return R.ggx_sample_table(roughness, samples, face_size, source_levels)
    if kind not in (LOBE_CHARLIE, LOBE_LAMBERT):
        raise ValueError("kind %r" % (kind,))
    S, N, L = int(samples), int(face_size), int(source_levels)
    xi1, phi = _points(S)
    if not 1 <= N <= R.MAX_FACE or not 1 <= L <= N.bit_length():
        raise ValueError("face_size %r, source_levels %r" % (face_size, source_levels))
    with np.errstate(divide="ignore"):
        if kind == LOBE_CHARLIE:
            r = float(np.float32(roughness))               # the C helper takes a float
            if not (0.0 < r <= 1.0):
                raise ValueError("roughness %r outside (0, 1]" % (roughness,))
            a = r*r
            sin = np.power(xi1, a/(2.0*a + 1.0))
            hz = np.sqrt(1.0 - sin*sin)
            hx = sin*np.cos(phi)
            hy = sin*np.sin(phi)
            lx = (2.0*hz)*hx
            ly = (2.0*hz)*hy
            lz = (2.0*hz)*hz - 1.0
            pdf = (((2.0 + 1.0/a)*np.power(sin, 1.0/a))/(2.0*PI))/4.0
        else:
            lz = 1.0 - xi1
            sin = np.sqrt(1.0 - lz*lz)
            lx = sin*np.cos(phi)
            ly = sin*np.sin(phi)
            pdf = np.full(S, 1.0/(2.0*PI))
        lod = 0.5*np.log2((1.0/(float(S)*pdf))/((4.0*PI)/(6.0*(float(N)*float(N))))) + 1.0
    lod = np.minimum(np.maximum(lod, 0.0), float(L - 1))
    below = lz <= 0.0
    lz = np.where(below, 0.0, lz)
    lod = np.where(below, 0.0, lod)
    return np.stack([lx, ly, lz, lod], -1).astype(np.float32)


def hammersley_table(samples: int) -> np.ndarray:
    """-> (samples, 4) float32 records (cos phi, sin phi, xi1, 0)"""
    xi1, phi = _points(samples)
    return np.stack([np.cos(phi), np.sin(phi), xi1, np.zeros_like(xi1)], -1).astype(np.float32)


def brdf_lut(width: int, height: int, table: np.ndarray, sheen: bool = False) -> np.ndarray:
    """-> (height, width, 4) float32: R, G the GGX scale and bias, B the Charlie albedo (0 without sheen), A 1"""
    w, h = int(width), int(height)
    tab = np.asarray(table, np.float32).astype(np.float64)
    S = tab.shape[0]
    assert 1 <= w <= MAX_LUT and 1 <= h <= MAX_LUT and S % 64 == 0 and R.MIN_SAMPLES <= S <= R.MAX_SAMPLES
    c = tab[:, 0][:, None, None]
    xi = tab[:, 2][:, None, None]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    NoV = ((x + 0.5)/float(w))[None]
    r = ((y + 0.5)/float(h))[None]
    alpha = r*r
    a2 = alpha*alpha
    vx = np.sqrt(1.0 - NoV*NoV)
    vz = NoV
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c2 = (1.0 - xi)/(1.0 + (a2 - 1.0)*xi)
        hz = np.sqrt(c2)
        st = np.sqrt(1.0 - c2)
        hx = st*c
        VoH = (vx*hx) + (vz*hz)
        NoL = (2.0*VoH)*hz - vz
        ok = (NoL > 0.0) & (VoH > 0.0)
        vis = 0.5/(NoL*np.sqrt((NoV*NoV)*(1.0 - a2) + a2) + NoV*np.sqrt((NoL*NoL)*(1.0 - a2) + a2))
        t = ((vis*VoH)*NoL)/hz
        m = 1.0 - VoH
        fc = ((m*m)*(m*m))*m
        A = np.where(ok, (1.0 - fc)*t, 0.0)
        B = np.where(ok, fc*t, 0.0)
        out[..., 0] = ((4.0*R.sum64(A))/float(S)).astype(np.float32)
        out[..., 1] = ((4.0*R.sum64(B))/float(S)).astype(np.float32)
        if sheen:
            hz = 1.0 - xi
            st = np.sqrt(1.0 - hz*hz)
            hx = st*c
            VoH = (vx*hx) + (vz*hz)
            NoL = (2.0*VoH)*hz - vz
            ok = (NoL > 0.0) & (VoH > 0.0)
            vn = 1.0/(4.0*((NoL + NoV) - NoL*NoV))
            d = ((2.0 + 1.0/alpha)*np.power(st, 1.0/alpha))/(2.0*PI)
            C = np.where(ok, ((vn*d)*NoL)*VoH, 0.0)
            out[..., 2] = (((8.0*PI)*R.sum64(C))/float(S)).astype(np.float32)
    return out


def cube_irradiance(record: np.ndarray, n: int, over_pi: bool = False) -> np.ndarray:
    """the 37 doubles of sh9 -> (6, n, n, 4) float32: per channel E = 0.0, E = E + (k_b Y_b) coeff[b][c] in the order of b,
    at the texel's normalised direction; divided by pi with over_pi"""
    k = np.asarray(record, np.float64)[:36].reshape(9, 4)
    x, y, z = R.texel_normals(int(n))
    band = [PI] + [(2.0*PI)/3.0]*3 + [PI/4.0]*5
    basis = R.sh_basis(x, y, z)
    acc = np.zeros(x.shape + (4,))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(9):
            acc = acc + (band[b]*basis[b])[..., None]*k[b]
        if over_pi:
            acc = acc/PI
        return acc.astype(np.float32)


# ---- the independent check of the lookup table ---------------------------------------------------------------------------
def brdf_quadrature(NoV: float, r: float, n_theta: int = 512, n_phi: int = 1024):
    """-> (A, B, C) at one N.V and roughness by the midpoint rule over light directions (theta, phi) of the upper
    hemisphere: the integral of D Vis F NoL d omega with F split as (1 - Fc) + Fc, and of the Charlie lobe
    D_c V_neubelt NoL.  Nothing here is importance-sampled; phi covers half the circle and counts twice (the integrand
    is even in phi for a view in the xz plane)."""
    alpha = r*r
    a2 = alpha*alpha
    th = (np.arange(n_theta) + 0.5)*(0.5*PI/n_theta)
    ph = (np.arange(n_phi) + 0.5)*(PI/n_phi)
    th, ph = np.meshgrid(th, ph, indexing="ij")
    dw = np.sin(th)*(0.5*PI/n_theta)*(PI/n_phi)*2.0
    l = np.stack([np.sin(th)*np.cos(ph), np.sin(th)*np.sin(ph), np.cos(th)], -1)
    v = np.array([np.sqrt(1.0 - NoV*NoV), 0.0, NoV])
    hvec = l + v
    hvec = hvec/np.linalg.norm(hvec, axis=-1, keepdims=True)
    NoL = l[..., 2]
    NoH = hvec[..., 2]
    VoH = hvec @ v
    D = a2/(PI*(NoH*NoH*(a2 - 1.0) + 1.0)**2)
    vis = 0.5/(NoL*np.sqrt(NoV*NoV*(1.0 - a2) + a2) + NoV*np.sqrt(NoL*NoL*(1.0 - a2) + a2))
    fc = (1.0 - VoH)**5
    base = D*vis*NoL*dw
    sinh = np.sqrt(np.maximum(0.0, 1.0 - NoH*NoH))
    Dc = (2.0 + 1.0/alpha)*sinh**(1.0/alpha)/(2.0*PI)
    Vc = 1.0/(4.0*(NoL + NoV - NoL*NoV))
    return float(((1.0 - fc)*base).sum()), float((fc*base).sum()), float((Dc*Vc*NoL*dw).sum())
