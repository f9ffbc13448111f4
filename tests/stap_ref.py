"""Restatement of the space-time null steering (gpsmi_nul_cfg.taps = T in {3, 5, 7}, include/gpsmi.h;
DESIGN.md 4.2o) in numpy: the contract the kernels of csrc/gpsmi_nul_stap.h are held to, a plain
evaluation of the same formulas (the yardstick of the tolerances), and the blocks of the tests.

Per block of n samples of A antennas, K = A T, c = (T - 1) / 2, k(a, t) = a T + t:
the lag sums r_ab(l) = sum_{i=l}^{n-1} x_a[i] conj(x_b[i - l]), the matrix R of the zero-extended shifted
rows, the loading, Cholesky without pivoting and the two triangular solves one float64 operation at a
time, w = u / Re u_{k(0,c)}, the decision, and y[i] = sum_a sum_t conj(w32[a][t]) x_a[i + c - t] in
float32 with the first and last c samples zero.

The header leaves the order of the lag sums open (the kernel's float64 matrix instruction does not
document its own), so StapRef evaluates them two ways and computes everything after them once from
each:
    'f64'   the four real sums RR, II, IR, RI of every (a, b, l) in ascending sample order in float64
            (np.cumsum adds one element at a time), re = RR + II, im = IR - RI.  With T = 1 the sums
            are nul_ref.covariance's instead: the documented order of the one-weight kernels, so that
            StapRef(T = 1) is nul_ref.NullRef byte for byte;
    'ext'   the same sums in extended precision: np.longdouble (the x87 80-bit format here, 64 bits
            of mantissa: every product of two float32 samples and, at these n, the sums carry 11
            more bits than float64), rounded to float64 once at the end.  Where np.longdouble is
            float64 the sums go through math.fsum instead, which is exact.
"""
import math

import numpy as np

import nul_ref as R
from nul_ref import cgauss, decode, f32, quantise, steer  # noqa: F401  (the tests take them from here)

_EXT_IS_WIDER = np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant


def rows16(x):
    """complex64 [A][n] -> float64 [2 A][n]: Re x_0 .. Re x_{A-1}, Im x_0 .. Im x_{A-1}."""
    x = np.asarray(x, dtype=np.complex64)
    return np.concatenate([x.real, x.imag]).astype(np.float64)


def tiles(v, T, mode='f64'):
    """v float64 [2 A][n] -> D [T][2 A][2 A], D[l][p][q] = sum_{i>=l} v_p[i] v_q[i - l] (every product
    is exact in float64): float64 in ascending sample order, or extended precision (np.longdouble)."""
    m, n = v.shape
    D = np.zeros((T, m, m), dtype=np.float64 if mode == 'f64' else np.longdouble)
    vt = np.ascontiguousarray(v.T)                   # [n][2 A]
    vl = v.astype(np.longdouble) if mode != 'f64' and _EXT_IS_WIDER else None
    for l in range(T):
        for p in range(m):
            if mode == 'f64':                        # (a sum over the outer axis adds row after row)
                D[l, p] = np.add.reduce(v[p, l:][:, None] * vt[:n - l], axis=0)
            elif _EXT_IS_WIDER:
                D[l, p] = (vl[p, l:][None, :] * vl[:, :n - l]).sum(axis=1)
            else:
                D[l, p] = [math.fsum(row.tolist()) for row in v[p, l:][None, :] * v[:, :n - l]]
    return D


def lag_sums(x, T, mode='f64'):
    """x complex64 [A][n] -> r complex128 [T][A][A], r[l][a][b] = sum_{i>=l} x_a[i] conj(x_b[i - l])
    (at l = 0 Hermitian, filled from a >= b, the diagonal's imaginary part exactly 0)."""
    x = np.asarray(x, dtype=np.complex64)
    A, n = x.shape
    r = np.zeros((T, A, A), dtype=np.complex128)
    if T == 1 and mode == 'f64':
        r[0] = R.covariance(x)
        return r
    D = tiles(rows16(x), T, mode)
    for l in range(T):
        for a in range(A):
            for b in range(a + 1 if l == 0 else A):
                re = float(D[l, a, b] + D[l, A + a, A + b])              # RR + II
                im = float(D[l, A + a, b] - D[l, a, A + b])              # IR - RI
                if l == 0 and a == b:
                    im = 0.0
                r[l, a, b] = complex(re, im)
                if l == 0 and a != b:
                    r[0, b, a] = complex(re, -im)
    return r


def lag_matrix(r, n):
    """r [T][A][A] -> R complex128 [K][K] before the loading: R[k(a,t)][k(b,s)] = r_ab(s - t) / n for
    s >= t, conj(r_ba(t - s)) / n for s < t; each component divided by n on its own."""
    T, A = r.shape[0], r.shape[1]
    K = A * T
    dn = float(n)
    M = np.zeros((K, K), dtype=np.complex128)
    for a in range(A):
        for t in range(T):
            for b in range(A):
                for s in range(T):
                    if s >= t:
                        z = r[s - t, a, b]
                        M[a * T + t, b * T + s] = complex(z.real / dn, z.imag / dn)
                    else:
                        z = r[t - s, b, a]
                        M[a * T + t, b * T + s] = complex(z.real / dn, -(z.imag / dn))
    return M


def solve(r, n, load=0.0, min_gain_db=0.0):
    """Lag sums of a block of n samples -> (w complex128 [A][T], flag, gain_db float32): every float64
    operation of the header one at a time (numpy float64 element operations and Python floats: IEEE
    double, nothing fused); with T = 1 the operations of nul_ref.solve in its order."""
    T, A = r.shape[0], r.shape[1]
    K, kc = A * T, (T - 1) // 2
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    min_db = f32(3.0) if f32(min_gain_db) == 0.0 else f32(min_gain_db)
    M = lag_matrix(r, n)
    Rr, Ri = M.real.copy(), M.imag.copy()
    tr = 0.0
    for a in range(A):
        tr += float(Rr[a * T, a * T])
    p00 = float(Rr[0, 0])
    delta = load * tr / float(A)
    for k in range(K):
        Rr[k, k] = Rr[k, k] + delta
        Ri[k, k] = 0.0
    Lr, Li = np.zeros((K, K)), np.zeros((K, K))
    e = np.zeros((A, T), dtype=np.complex128)
    e[0, kc] = 1.0
    ok = True
    with np.errstate(all='ignore'):
        for j in range(K):
            d = float(Rr[j, j])
            for k in range(j):
                d -= float(Lr[j, k]) * float(Lr[j, k]) + float(Li[j, k]) * float(Li[j, k])
            if not (d > 0.0) or not (d < np.inf):
                ok = False
            l = np.sqrt(np.float64(d))
            Lr[j, j], Li[j, j] = l, 0.0
            vr, vi = Rr[j + 1:, j].copy(), Ri[j + 1:, j].copy()
            for k in range(j):                       # v -= L[i][k] conj(L[j][k]), ascending k
                ar, ai, br, bi = Lr[j + 1:, k], Li[j + 1:, k], Lr[j, k], -Li[j, k]
                vr = vr - (ar * br - ai * bi)
                vi = vi - (ar * bi + ai * br)
            Lr[j + 1:, j], Li[j + 1:, j] = vr / l, vi / l
        if not ok:
            return e, 0, np.float32(0.0)
        # L y = e_kc: every row subtracts its terms in ascending column order
        vr, vi = np.zeros(K), np.zeros(K)
        vr[kc] = 1.0
        yr, yi = np.zeros(K), np.zeros(K)
        for k in range(K):
            yr[k], yi[k] = vr[k] / Lr[k, k], vi[k] / Lr[k, k]
            ar, ai = Lr[k + 1:, k], Li[k + 1:, k]
            vr[k + 1:] = vr[k + 1:] - (ar * yr[k] - ai * yi[k])
            vi[k + 1:] = vi[k + 1:] - (ar * yi[k] + ai * yr[k])
        # L^H u = y: rows descending, ascending column order within a row
        u = [None] * K
        for i in range(K - 1, -1, -1):
            v = (float(yr[i]), float(yi[i]))
            for k in range(i + 1, K):
                v = R._sub(v, R._mul((float(Lr[k, i]), -float(Li[k, i])), u[k]))
            u[i] = R._div(v, float(Lr[i, i]))
        gdb = float(10.0 * np.log10(np.float64(p00 * u[kc][0])))
    if not (gdb >= min_db):
        return e, 0, np.float32(gdb)
    w = np.zeros(K, dtype=np.complex128)
    for k in range(K):
        w[k] = complex(u[k][0] / u[kc][0], u[k][1] / u[kc][0])
    w[kc] = 1.0
    return w.reshape(A, T), 1, np.float32(gdb)


def combine(x, w):
    """y[i] = sum_a sum_t conj(w32[a][t]) x_a[i + c - t] for c <= i < n - c in float32, ascending a,
    ascending t within a, from (0, 0)'s term, nothing fused; +0.0 + 0.0j in the first and last c."""
    x = np.asarray(x, dtype=np.complex64)
    w32 = np.asarray(w, dtype=np.complex128).astype(np.complex64)
    if w32.ndim == 1:
        w32 = w32[:, None]
    A, n = x.shape
    T = w32.shape[1]
    c = (T - 1) // 2
    yr = yi = None
    for a in range(A):
        for t in range(T):
            wr, wi = w32[a, t].real, w32[a, t].imag    # (np.float32 scalars)
            seg = x[a, 2 * c - t:n - t]
            xr, xi = seg.real, seg.imag
            tr = wr * xr + wi * xi
            ti = wr * xi - wi * xr
            yr, yi = (tr, ti) if yr is None else (yr + tr, yi + ti)
    out = np.zeros(n, dtype=np.complex64)
    out.real[c:n - c], out.imag[c:n - c] = yr, yi
    return out


class StapRef:
    def __init__(self, n, antennas, taps, load=0.0, min_gain_db=0.0):
        self.n, self.A, self.T = n, antennas, max(1, taps)
        self.load, self.min_gain_db = load, min_gain_db

    def process(self, x, mode='f64'):
        """One block (complex64 [A][n]) -> (y complex64 [n], flag, gain_db float32, w complex128 [A][T])."""
        x = np.asarray(x, dtype=np.complex64)
        assert x.shape == (self.A, self.n)
        w, flag, g = solve(lag_sums(x, self.T, mode), self.n, self.load, self.min_gain_db)
        y = combine(x, w) if flag else x[0].copy()
        return y, flag, g, w

    def run(self, x, mode='f64'):
        """[A][nb * n] complex64 (or uint16: decoded first) -> (y [nb][n], flags int32 [nb], gain_db
        float32 [nb], weights complex128 [nb][A][T])."""
        x = np.asarray(x)
        if x.dtype == np.uint16:
            x = decode(x)
        x = x.reshape(self.A, -1, self.n)
        res = [self.process(x[:, b], mode) for b in range(x.shape[1])]
        return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32),
                np.array([r[2] for r in res], dtype=np.float32), np.stack([r[3] for r in res]))


def shifted_rows(x, T):
    """Z complex128 [A T][n + T - 1]: Z[k(a,t)][i] = x_a[i - t], zero outside the block."""
    x = np.asarray(x, dtype=np.complex64).astype(np.complex128)
    A, n = x.shape
    Z = np.zeros((A * T, n + T - 1), dtype=np.complex128)
    for a in range(A):
        for t in range(T):
            Z[a * T + t, t:t + n] = x[a]
    return Z


def plain(x, n, T, load=0.0, min_gain_db=0.0):
    """The header's formulas as one would write them in numpy, no order kept: the Gram matrix of the
    shifted rows as a matrix product, a general solve, a complex64 weighted sum.  One block [A][n] ->
    (y, flag, gain_db, w [A][T])."""
    x = np.asarray(x, dtype=np.complex64)
    A = x.shape[0]
    K, c = A * T, (T - 1) // 2
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    min_db = f32(3.0) if f32(min_gain_db) == 0.0 else f32(min_gain_db)
    Z = shifted_rows(x, T)
    G = Z @ Z.conj().T / n
    e = np.zeros(K, dtype=np.complex128)
    e[c] = 1.0
    Rm = G + load * sum(G[a * T, a * T].real for a in range(A)) / A * np.eye(K)
    with np.errstate(all='ignore'):
        try:
            np.linalg.cholesky(Rm)
            u = np.linalg.solve(Rm, e)
            gdb = 10.0 * np.log10(G[0, 0].real * u[c].real)
        except np.linalg.LinAlgError:
            return x[0].copy(), 0, np.float32(0.0), e.reshape(A, T)
    if not (gdb >= min_db):
        return x[0].copy(), 0, np.float32(gdb), e.reshape(A, T)
    w = u / u[c].real
    w[c] = 1.0
    w = w.reshape(A, T)
    w32 = w.astype(np.complex64)
    y = np.zeros(n, dtype=np.complex64)
    terms = np.stack([np.conj(w32[a, t]) * x[a, 2 * c - t:n - t] for a in range(A) for t in range(T)])
    y[c:n - c] = terms.sum(axis=0, dtype=np.complex64)
    return y, 1, np.float32(gdb), w


# ---- blocks of the tests ------------------------------------------------------------------------

def jammer(rng, A, n, amp, kind):
    """complex128 [A][n]: one jammer of power amp^2 per antenna from a random direction, with temporal
    structure.  'tone': a carrier at a random frequency.  'filtered': white noise through a two-tap
    filter of its own per antenna (1, h_a), |h_a| = 0.3 .. 0.7 at a random phase: the channels differ
    by more than a phase, and every lag up to 1 carries signal."""
    st = steer(rng, A)
    if kind == 'tone':
        f, ph = rng.uniform(-0.4, 0.4), rng.uniform(0.0, 2.0 * np.pi)
        return st[:, None] * (amp * np.exp(1j * (2.0 * np.pi * f * np.arange(n) + ph)))[None, :]
    z = cgauss(rng, n + 1)
    h = rng.uniform(0.3, 0.7, A) * np.exp(2j * np.pi * rng.random(A))
    rows = [(z[1:] + h[a] * z[:-1]) / np.sqrt(1.0 + abs(h[a]) ** 2) for a in range(A)]
    return st[:, None] * amp * np.stack(rows)


def stap_block(rng, A, n, jammers=0, jn_db=20.0, sigma=0.015, first='filtered'):
    """complex128 [A][n]: independent noise of power sigma^2 per antenna and `jammers` jammers jn_db above
    it, alternating between the two kinds from `first`."""
    x = sigma * cgauss(rng, (A, n))
    kinds = ('filtered', 'tone') if first == 'filtered' else ('tone', 'filtered')
    for j in range(jammers):
        x = x + jammer(rng, A, n, sigma * 10.0 ** (jn_db / 20.0), kinds[j % 2])
    return x


# ---- scenes: what the taps buy --------------------------------------------------------------------

A2 = 2
DELAY = 0.3                                  # samples between the two channels
JAM_SINE = 0.5
TONES = (-510e3, -470e3, -430e3)             # a tone field, each tone from a direction of its own
TONE_SINES = (-0.6, 0.1, 0.75)
LEVELS = {('a', False): 40.0, ('a', True): 30.0, ('b', False): 35.0, ('b', True): 25.0}
_SCENES = {}
# what StapRef followed by the oracle's sweep acquires (tests/test_stap.py determines it on the CPU):
# (scene, raw_u8, taps) -> PRN -> (bin, code phase).  PRNs 4 and 24 stand 7 and 10 degrees from the
# white jammer and go with it (two antennas: one broad null); the tones leave every direction open.
_WHITE = {6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963), 28: (-2000.0, 1877), 32: (-2200.0, 1714)}
_TONES = {4: (-2000.0, 143), 6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963), 24: (-2800.0, 150),
          27: (-3800.0, 1305), 28: (-2000.0, 1876), 32: (-2200.0, 1714)}
FOUND = {('a', False, 1): {}, ('a', True, 1): {}, ('b', False, 1): {}, ('b', True, 1): {},
         ('a', False, 5): {**_WHITE, 27: (-3800.0, 1305)}, ('a', True, 5): {**_WHITE, 27: (-3600.0, 1305)},
         ('b', False, 5): _TONES, ('b', True, 5): _TONES}


def stap_scene(kind, raw_u8=True):
    """Eight satellites seen by two antennas half a wavelength apart whose channels differ by a delay
    of 0.3 samples (a windowed sinc).  'a': one white jammer, 40 dB over the noise of an antenna for
    complex64 and 30 dB for the 8-bit rendering (the highest level at which the noise keeps 1.6 LSB
    under the clipping limit).  'b': three tones from three directions, 35 / 25 dB each.  'clean': no
    jammer.  raw_u8 picks the level; block() / block_raw() render 8 bits, block_c64() complex64."""
    from gpsmi import synth, synth_array as SA
    key = (kind, bool(raw_u8) or kind == 'clean')
    if key not in _SCENES:
        sc = synth.default_scene(8, seed=7)
        st = SA.ula_steering(A2, np.linspace(-0.9, 0.9, 8))
        if kind == 'a':
            jam = [SA.Jammer(steering=SA.ula_steering(A2, [JAM_SINE])[:, 0], jn_db=LEVELS[key])]
        elif kind == 'b':
            jam = [SA.Jammer(steering=SA.ula_steering(A2, [sn])[:, 0], jn_db=LEVELS[key], kind='tones',
                             tones=[f], stream=500 + 10 * i) for i, (sn, f) in enumerate(zip(TONE_SINES, TONES))]
        else:
            jam = []
        _SCENES[key] = SA.ArrayScene(sc, st, jam, channel=[None, DELAY])
    return _SCENES[key]


def block_c64(arr, b):
    """Block b without the 8-bit rendering: complex64 of the float samples."""
    return arr.block_float(b).astype(np.complex64)


def oracle_sweep(blocks):
    """The oracle's acquisition sweep (gps_oracle.sweep_all_sats, 10 bins per block) over blocks(i)
    -> {PRN: (bin, code phase)}."""
    import gps_oracle as orc
    from gpsmi import synth
    p = orc.Params()
    prns = [s.prn for s in synth.default_scene(8, seed=7).sats] + [1]
    spectra = {s: orc.fft_cacode(s, p.code_samples) for s in prns}
    t = orc.sec_time(p)
    freq, lst, found, ready, i = p.min_freq, list(prns), [], False, 0
    while not ready:
        ready, freq, found = orc.sweep_all_sats(blocks(i), freq, lst, found, p.it_sweep_all, p, spectra, t)
        i += 1
    return {s: (f, d) for _, s, f, d in found}


def filt(x, w):
    """complex128 y[i] = sum_a sum_t conj(w[a][t]) x_a[i + c - t] on c <= i < n - c (no rounding kept)."""
    w = np.asarray(w, dtype=np.complex128)
    if w.ndim == 1:
        w = w[:, None]
    A, T = w.shape
    n, c = x.shape[1], (T - 1) // 2
    return sum(np.conj(w[a, t]) * x[a, 2 * c - t:n - t] for a in range(A) for t in range(T))
