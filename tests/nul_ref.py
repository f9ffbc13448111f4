"""float64 restatement of the null steering (gpsmi_nul_*, include/gpsmi.h): the contract the HIP
kernels of csrc/gpsmi_nul.hip are held to, a plain numpy evaluation of the same formulas (the
yardstick of the tolerances), and the scenes of the tests.

Per block of n samples of A antennas: the covariance C[a][b] = sum_i x_a[i] conj(x_b[i]) in float64
in the header's order (slices of 8192 samples; lane t of 256 takes the samples 2048 r + 8 t .. + 7,
r = 0 .. 3; the lane sums as a tree of neighbours; the slices in ascending order),
R = C / n + delta I, Cholesky without pivoting and the two triangular solves one operation at a time,
w = u / Re u[0], the decision, and y = sum_a conj(w32[a]) x_a in float32, nothing fused.
"""
import numpy as np

SLICE, GROUP, LANES = 8192, 8, 256


def f32(v):
    return float(np.float32(v))


def decode(raw):
    """uint16 (Q << 8 | I) -> complex64 as decode_u8iq: float32(byte) * float32(1 / 127.5) - 1."""
    raw = np.asarray(raw, dtype=np.uint16)
    scl = np.float32(1.0) / np.float32(127.5)
    re = (raw & 0xFF).astype(np.float32) * scl - np.float32(1.0)
    im = (raw >> 8).astype(np.float32) * scl - np.float32(1.0)
    out = np.empty(raw.shape, dtype=np.complex64)
    out.real, out.imag = re, im
    return out


def pairs(A):
    """(a, b) with a >= b in the order of the packed covariance: p = a (a + 1) / 2 + b."""
    return [(a, b) for a in range(A) for b in range(a + 1)]


def covariance(x):
    """x complex64 [A][n] -> C complex128 [A][A] (Hermitian, filled from the lower triangle), the
    sums in the header's order."""
    x = np.asarray(x, dtype=np.complex64)
    A, n = x.shape
    ns = -(-n // SLICE)
    pad = np.zeros((A, ns * SLICE), dtype=np.complex64)
    pad[:, :n] = x                                   # (a lane without samples adds nothing: +0.0)
    v = pad.reshape(A, ns, SLICE // (GROUP * LANES), LANES, GROUP)
    xr, xi = v.real.astype(np.float64), v.imag.astype(np.float64)
    ia = np.array([a for a, _ in pairs(A)])
    ib = np.array([b for _, b in pairs(A)])
    re = np.zeros((len(ia), ns, LANES))
    im = np.zeros((len(ia), ns, LANES))
    for r in range(v.shape[2]):
        for k in range(GROUP):
            ar, ai = xr[ia, :, r, :, k], xi[ia, :, r, :, k]
            br, bi = xr[ib, :, r, :, k], xi[ib, :, r, :, k]
            re = re + ar * br
            re = re + ai * bi
            im = im + ai * br
            im = im - ar * bi
    for _ in range(8):                               # lanes 2k + (2k + 1), then pairs of those, ...
        re = re[..., 0::2] + re[..., 1::2]
        im = im[..., 0::2] + im[..., 1::2]
    re, im = re[..., 0], im[..., 0]                  # [pairs][slices]
    cr, ci = re[:, 0].copy(), im[:, 0].copy()
    for s in range(1, ns):
        cr = cr + re[:, s]
        ci = ci + im[:, s]
    C = np.zeros((A, A), dtype=np.complex128)
    for p, (a, b) in enumerate(pairs(A)):
        if a == b:
            C[a, a] = cr[p]
        else:
            C[a, b] = complex(cr[p], ci[p])
            C[b, a] = complex(cr[p], -ci[p])
    return C


def _mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _conj(a):
    return (a[0], -a[1])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def solve(C, n, load=0.0, min_gain_db=0.0):
    """C [A][A] of a block of n samples -> (w complex128 [A], flag, gain_db float32), every float64
    operation in the header's order (Python floats: IEEE double, nothing fused)."""
    A = C.shape[0]
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    min_db = f32(3.0) if f32(min_gain_db) == 0.0 else f32(min_gain_db)
    dn = float(n)
    R = [[(float(C[a, b].real) / dn, 0.0 if a == b else float(C[a, b].imag) / dn) for b in range(a + 1)]
         for a in range(A)]
    tr = 0.0
    for a in range(A):
        tr += R[a][a][0]
    p00 = R[0][0][0]
    delta = load * tr / float(A)
    for a in range(A):
        R[a][a] = (R[a][a][0] + delta, 0.0)
    L = [[None] * A for _ in range(A)]
    ok = True
    with np.errstate(all='ignore'):
        for j in range(A):
            d = R[j][j][0]
            for k in range(j):
                d -= L[j][k][0] * L[j][k][0] + L[j][k][1] * L[j][k][1]
            if not (d > 0.0) or not (d < np.inf):
                ok = False
            l = float(np.sqrt(np.float64(d)))
            L[j][j] = (l, 0.0)
            for i in range(j + 1, A):
                v = R[i][j]
                for k in range(j):
                    v = _sub(v, _mul(L[i][k], _conj(L[j][k])))
                L[i][j] = _div(v, l)
        e0 = np.zeros(A, dtype=np.complex128)
        e0[0] = 1.0
        if not ok:
            return e0, 0, np.float32(0.0)
        y = [None] * A
        u = [None] * A
        y[0] = (1.0 / L[0][0][0], 0.0)
        for i in range(1, A):
            v = (0.0, 0.0)
            for k in range(i):
                v = _sub(v, _mul(L[i][k], y[k]))
            y[i] = _div(v, L[i][i][0])
        for i in range(A - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, A):
                v = _sub(v, _mul(_conj(L[k][i]), u[k]))
            u[i] = _div(v, L[i][i][0])
        gdb = float(10.0 * np.log10(np.float64(p00 * u[0][0])))
    if not (gdb >= min_db):
        return e0, 0, np.float32(gdb)
    w = e0.copy()
    for a in range(1, A):
        w[a] = complex(u[a][0] / u[0][0], u[a][1] / u[0][0])
    return w, 1, np.float32(gdb)


def _div(v, l):
    with np.errstate(all='ignore'):
        return (float(np.float64(v[0]) / np.float64(l)), float(np.float64(v[1]) / np.float64(l)))


def combine(x, w):
    """y = sum_a conj(w32[a]) x_a in float32, ascending a from antenna 0's term, nothing fused."""
    x = np.asarray(x, dtype=np.complex64)
    w32 = np.asarray(w, dtype=np.complex128).astype(np.complex64)
    yr = yi = None
    for a in range(x.shape[0]):
        wr, wi = w32[a].real, w32[a].imag           # (np.float32 scalars)
        xr, xi = x[a].real, x[a].imag
        tr = wr * xr + wi * xi
        ti = wr * xi - wi * xr
        yr, yi = (tr, ti) if a == 0 else (yr + tr, yi + ti)
    out = np.empty(x.shape[1], dtype=np.complex64)
    out.real, out.imag = yr, yi
    return out


class NullRef:
    def __init__(self, n, antennas, load=0.0, min_gain_db=0.0):
        self.n, self.A, self.load, self.min_gain_db = n, antennas, load, min_gain_db

    def process(self, x):
        """One block (complex64 [A][n]) -> (y complex64 [n], flag, gain_db float32, w complex128 [A])."""
        x = np.asarray(x, dtype=np.complex64)
        assert x.shape == (self.A, self.n)
        w, flag, g = solve(covariance(x), self.n, self.load, self.min_gain_db)
        y = combine(x, w) if flag else x[0].copy()
        return y, flag, g, w

    def run(self, x):
        """[A][nb * n] complex64 (or uint16: decoded first) -> (y [nb][n], flags int32 [nb], gain_db
        float32 [nb], weights complex128 [nb][A])."""
        x = np.asarray(x)
        if x.dtype == np.uint16:
            x = decode(x)
        x = x.reshape(self.A, -1, self.n)
        res = [self.process(x[:, b]) for b in range(x.shape[1])]
        return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32),
                np.array([r[2] for r in res], dtype=np.float32), np.stack([r[3] for r in res]))


def plain(x, n, load=0.0, min_gain_db=0.0):
    """The header's formulas as one would write them in numpy, no order kept: a matrix product, a
    general solve, a complex64 weighted sum.  One block [A][n] -> (y, flag, gain_db, w).  Its
    distance from NullRef is what float64 and float32 leave open, the yardstick of the GPU tests."""
    x = np.asarray(x, dtype=np.complex64)
    A = x.shape[0]
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    min_db = f32(3.0) if f32(min_gain_db) == 0.0 else f32(min_gain_db)
    X = x.astype(np.complex128)
    C = X @ X.conj().T / n
    e0 = np.zeros(A, dtype=np.complex128)
    e0[0] = 1.0
    R = C + load * np.trace(C).real / A * np.eye(A)
    with np.errstate(all='ignore'):
        try:
            np.linalg.cholesky(R)
            u = np.linalg.solve(R, e0)
            gdb = 10.0 * np.log10(C[0, 0].real * u[0].real)
        except np.linalg.LinAlgError:
            return x[0].copy(), 0, np.float32(0.0), e0
    if not (gdb >= min_db):
        return x[0].copy(), 0, np.float32(gdb), e0
    w = u / u[0].real
    w[0] = 1.0
    y = (np.conj(w.astype(np.complex64))[:, None] * x).sum(axis=0, dtype=np.complex64)
    return y, 1, np.float32(gdb), w


# ---- scenes ------------------------------------------------------------------------------------

def cgauss(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def steer(rng, A):
    """A random phase per antenna, antenna 0 at phase 0."""
    ph = 2.0 * np.pi * rng.random(A)
    ph[0] = 0.0
    return np.exp(1j * ph)


def noisy_block(rng, A, n, jammers=0, jn_db=30.0, sigma=0.02):
    """complex128 [A][n]: independent noise of power sigma^2 per antenna and `jammers` white jammers
    jn_db above it from random directions."""
    x = sigma * cgauss(rng, (A, n))
    for _ in range(jammers):
        x = x + steer(rng, A)[:, None] * (sigma * 10.0 ** (jn_db / 20.0)) * cgauss(rng, n)[None, :]
    return x


def quantise(x):
    """complex128 -> the recorder's uint16 (Q << 8 | I)."""
    i = np.clip(np.rint((x.real + 1.0) * 127.5), 0, 255).astype(np.uint16)
    q = np.clip(np.rint((x.imag + 1.0) * 127.5), 0, 255).astype(np.uint16)
    return (q << 8) | i


A4 = 4
JAM_SINE, JN_DB = 0.33, 30.0
_SCENES = {}


def array_scene(jammed=True):
    """Eight satellites spread over the sky of a four-antenna line (half a wavelength apart), and one
    white jammer 30 dB over the noise of an antenna."""
    from gpsmi import synth, synth_array as SA
    if jammed not in _SCENES:
        sc = synth.default_scene(8, seed=7)
        st = SA.ula_steering(A4, np.linspace(-0.9, 0.9, 8))
        jam = [SA.Jammer(steering=SA.ula_steering(A4, [JAM_SINE])[:, 0], jn_db=JN_DB)] if jammed else []
        _SCENES[jammed] = SA.ArrayScene(sc, st, jam)
    return _SCENES[jammed]
