"""Float64 numpy restatement of the acquisition searches (gpsmi_acq_search*, gpsmi_acq_search_nc,
gpsmi_acq_search_deep; csrc/gpsmi_acq_search.h and the correlations of gpsmi_pfa.h, gpsmi_bigfft.h,
gpsmi_direct.h), shared by test_acq_ref.py (CPU) and test_gpu_acq_ref.py (GPU).  Written from
include/gpsmi.h and the header comment of gpsmi_acq_search.h; nothing of the oracle's float32 path
is used by the reference itself.

For iq (complex64, or the recorder's uint16 decoded by corr_ref.decode_u8), Doppler bins f, PRNs and
(n_coh, n_seg, shifts), with cs samples per code period:
    om      = float32(2 pi f): the double product rounded once
    t32[k]  = float32(k + 1) / float32(1000 cs), divided in float32
    p[k]    = float32(om t32[k])
            -- these three float32 values are inputs of the operation, not errors of it: the
               reference fixes the phase argument in float32 and the kernels reproduce it.
               Everything below is float64 / complex128.
    wiped   = x exp(-j p)
    fold_s  = mean of the n_coh code periods of segment s; the phase restarts at t32[0] in every
              segment
    corr_s[n] = |sum_m fold_s[m] rep[(m - n) mod cs]|            (complex128 FFT of length cs)
    S[i]    = (1 / n_seg) sum_s corr_s[(i + m[b][s]) mod cs]     (m = 0: coherent, non-coherent)
    record  = first-index argmax, peak, mean, population std, lo = S[argmax - 1], hi = S[argmax + 1]
              (circular), and what the tests scale and excuse by: rms = sqrt(mean(S^2)),
              gap = (largest - second largest) / largest (0 on an all-zero surface).
rep is codes.code_replica(prn, cs) unless the caller hands over the replicas it uploaded (`reps`).

Beside it: three float32 restatements that the GPU tests measure their bounds with (oracle_record,
oracle_record_padded, direct_bound), the exact record of integer-valued inputs
(exact_integer_record), and the seeded inputs of test_gpu_acq_ref.py, so that the CPU file can hold
them to the near-tie caps without a GPU."""
import numpy as np

from corr_ref import decode_u8

L1_HZ = 1575.42e6
NEAR_TIE = 1e-4                       # top-two gap at or below which the argmax is not determined
BIG_N = 32768                         # the zero-padded transform length of gpsmi_bigfft.h

REC_DTYPE = np.dtype([
    ('argmax', np.int32), ('peak', np.float64), ('mean', np.float64), ('std', np.float64),
    ('lo', np.float64), ('hi', np.float64), ('rms', np.float64), ('gap', np.float64)])
FIELDS = ('argmax', 'peak', 'mean', 'std', 'lo', 'hi')


# ---- the float32 inputs of the operation ---------------------------------------------------

def time_base(cs, n):
    """t32[k] = float32(k + 1) / float32(1000 cs), k < n."""
    return np.arange(1, n + 1, dtype=np.float32) / np.float32(1000 * cs)


def omega_f32(f):
    return np.float32(2.0 * np.pi * float(f))


def phase_arg(f, cs, n):
    """p[k] = float32(om t32[k]) as float64."""
    p = omega_f32(f) * time_base(cs, n)
    assert p.dtype == np.float32
    return p.astype(np.float64)


def _c64(iq):
    x = np.asarray(iq)
    return decode_u8(x) if x.dtype == np.uint16 else x


def replica(prn, cs, reps=None):
    """The real replica of a PRN, float64 [cs]: GPSCacode, or the vector the test uploaded."""
    if reps is not None:
        return np.asarray(reps[int(prn)], np.float64)
    from gpsmi import codes
    return codes.code_replica(int(prn), cs)


def deep_shifts(freqs, n_coh, n_seg, cs, carrier_hz=L1_HZ, f_offset=0.0):
    """m[b][s] mod cs of gpsmi.h in 0 .. cs - 1, int64 [nbins, n_seg]: float64 in the order
    written there, halves to even."""
    out = np.zeros((len(freqs), n_seg), np.int64)
    for b, f in enumerate(freqs):
        for s in range(n_seg):
            m = np.rint(-(np.float64(f) - f_offset) / carrier_hz * np.float64(s) * np.float64(n_coh)
                        * np.float64(cs))
            out[b, s] = int(np.fmod(m, cs)) % cs
    return out


# ---- the operation in float64 --------------------------------------------------------------

def fold(iq, f, cs, n_coh, seg=0):
    """complex128 [cs]: the wiped mean of the n_coh code periods of segment seg."""
    span = n_coh * cs
    x = _c64(iq)[seg * span:(seg + 1) * span].astype(np.complex128)
    assert x.shape == (span,)
    wiped = x * np.exp(-1j * phase_arg(f, cs, span))
    return wiped.reshape(n_coh, cs).sum(axis=0) / n_coh


def corr_mag(fold_spec, rep_spec):
    """|sum_m fold[m] rep[(m - n) mod cs]| from the two length-cs spectra (rep real)."""
    return np.abs(np.fft.ifft(fold_spec * np.conj(rep_spec)))


def rotated_mean(corrs, shifts=None):
    """S[i] = (1 / n_seg) sum_s corr_s[(i + m_s) mod cs]."""
    acc = np.zeros_like(corrs[0])
    for s, c in enumerate(corrs):
        m = 0 if shifts is None else int(shifts[s])
        acc = acc + (np.roll(c, -m) if m else c)
    return acc / len(corrs)


def record(S):
    """The REC_DTYPE record of a surface."""
    S = np.asarray(S, np.float64)
    n = len(S)
    r = np.zeros((), REC_DTYPE)
    mx = int(np.argmax(S))
    r['argmax'], r['peak'], r['mean'], r['std'] = mx, S[mx], np.mean(S), np.std(S)
    r['lo'], r['hi'] = S[(mx - 1) % n], S[(mx + 1) % n]
    r['rms'] = np.sqrt(np.mean(S * S))
    second = np.max(np.delete(S, mx))
    r['gap'] = (S[mx] - second) / S[mx] if S[mx] > 0 else 0.0
    return r


def _tables(per_cell, freqs, prns, surfaces):
    out = np.zeros((len(freqs), len(prns)), REC_DTYPE)
    for b in range(len(freqs)):
        for j in range(len(prns)):
            S = per_cell(b, j)
            out[b, j] = record(S)
            if surfaces is not None and out[b, j]['gap'] <= NEAR_TIE:
                surfaces[b, j] = np.asarray(S, np.float64)
    return out


def acq_ref(iq, freqs, prns, cs, n_coh, n_seg=1, shifts=None, reps=None, surfaces=None):
    """REC_DTYPE [nbins, nsv]: the float64 records of a search.  shifts: None, or int
    [nbins, n_seg] (the deep search).  surfaces: a dict that receives {(bin, sv): S} for the cells
    whose two largest lags are within NEAR_TIE of each other."""
    rspec = [np.fft.fft(replica(p, cs, reps)) for p in prns]
    fspec = [[np.fft.fft(fold(iq, f, cs, n_coh, s)) for s in range(n_seg)] for f in freqs]

    def cell(b, j):
        return rotated_mean([corr_mag(fs, rspec[j]) for fs in fspec[b]],
                            None if shifts is None else shifts[b])
    return _tables(cell, freqs, prns, surfaces)


# ---- float32 restatements: what the GPU tests take their bounds from -------------------------

def _oracle_wiped(iq, f, cs, n_coh, seg, t):
    import gps_oracle as orc
    span = n_coh * cs
    wiped, _ = orc.demod_doppler(_c64(iq)[seg * span:(seg + 1) * span], float(f), 0, span, t)
    assert wiped.dtype == np.complex64
    return wiped


def _oracle_record(surf):
    """record() with the oracle's own float32 statistics (peak_stats) where it has them."""
    import gps_oracle as orc
    r = record(surf)
    assert np.asarray(surf).dtype == np.float32
    mx, peak, mean, std = orc.peak_stats(surf)
    assert mx == r['argmax']
    r['peak'], r['mean'], r['std'] = peak, mean, std
    return r


def _oracle_tables(per_cell, freqs, prns):
    out = np.zeros((len(freqs), len(prns)), REC_DTYPE)
    for b in range(len(freqs)):
        for j in range(len(prns)):
            out[b, j] = _oracle_record(per_cell(b, j))
    return out


def _sum_segments(corrs, shifts, cs):
    """The sums of nc_table / deep_table: float32 accumulator, ascending segments, each row
    rotated by its shift, scaled by float32(1 / n_seg)."""
    acc = np.zeros(cs, np.float32)
    for s, c in enumerate(corrs):
        m = 0 if shifts is None else int(shifts[s])
        acc = acc + (np.roll(c, -m) if m % cs else c)
    return acc * np.float32(1.0 / len(corrs))


def _oracle_replica_spectrum(prn, cs, reps):
    """complex64: the replica as a handle holds it.  At 2048 samples the spectrum it is given
    (float64 FFT rounded to complex64, AcqEngine); elsewhere the float32 FFT of the float32 replica
    it is given.  With a complex64 spectrum circ_corr and everything behind it run in float32; with
    fft_cacode's complex128 one (as acq_table calls it) the product, the inverse transform, |.| and
    the statistics run in float64 and only the wipe-off and the forward transform are float32."""
    import gps_oracle as orc
    rep = replica(prn, cs, reps)
    spec = np.fft.fft(rep).astype(np.complex64) if cs == 2048 else orc.fft(rep.astype(np.float32))
    assert spec.dtype == np.complex64
    return spec


def oracle_record(iq, freqs, prns, cs, n_coh, n_seg=1, shifts=None, reps=None):
    """The same records from gps_oracle's float32 functions: demod_doppler, folded_spectrum,
    circ_corr (on the complex64 replica spectrum: see above), and the sums of nc_table /
    deep_table, peak_stats on the float32 surface."""
    import gps_oracle as orc
    t = time_base(cs, n_coh * cs)
    rspec = [_oracle_replica_spectrum(p, cs, reps) for p in prns]
    fspec = [[orc.folded_spectrum(_oracle_wiped(iq, f, cs, n_coh, s, t), 0, n_coh, cs) for s in range(n_seg)]
             for f in freqs]

    def cell(b, j):
        return _sum_segments([orc.circ_corr(fs, rspec[j]) for fs in fspec[b]],
                             None if shifts is None else shifts[b], cs)
    return _oracle_tables(cell, freqs, prns)


def oracle_fold(iq, f, cs, n_coh, seg=0):
    """complex64 [cs]: the oracle's wiped samples folded in the time domain, in float32."""
    w = _oracle_wiped(iq, f, cs, n_coh, seg, time_base(cs, n_coh * cs))
    acc = np.zeros(cs, np.complex64)
    for i in range(n_coh):
        acc = acc + w[i * cs:(i + 1) * cs]
    out = acc / np.float32(n_coh)
    assert out.dtype == np.complex64
    return out


def oracle_record_padded(iq, freqs, prns, cs, n_coh, n_seg=1, shifts=None, reps=None):
    """oracle_record with the correlation taken through a zero-padded 32768-point float32
    transform pair, corr[n] = |lin[n] + lin[n - L]|: the arithmetic class of gpsmi_bigfft.h,
    in numpy."""
    from scipy.fft import fft, ifft
    assert 2 * cs - 1 <= BIG_N

    def padded(v, dtype):
        z = np.zeros(BIG_N, dtype)
        z[:cs] = v
        return fft(z)
    rspec = [padded(replica(p, cs, reps).astype(np.float32), np.float32) for p in prns]
    fspec = [[padded(oracle_fold(iq, f, cs, n_coh, s), np.complex64) for s in range(n_seg)] for f in freqs]
    assert rspec[0].dtype == np.complex64 and fspec[0][0].dtype == np.complex64

    def corr(fs, rs):
        lin = ifft(fs * np.conj(rs))
        assert lin.dtype == np.complex64
        return np.abs(lin[:cs] + lin[BIG_N - cs:BIG_N - cs + cs])

    def cell(b, j):
        return _sum_segments([corr(fs, rspec[j]) for fs in fspec[b]],
                             None if shifts is None else shifts[b], cs)
    return _oracle_tables(cell, freqs, prns)


def direct_bound(iq, f, prn, cs, n_coh, reps=None):
    """float64 [cs]: how far a magnitude of the time-domain correlation (acq_fold_kernel +
    circ_corr_direct_kernel) may be from the float64 one, per lag n:
        gamma sum_m |fold[m]| |rep[(m - n) mod L]| + E_fold,
    gamma = L 2^-24, the forward bound of L float32 FMAs accumulated in any order, and E_fold the
    float32 oracle fold's worst deviation from the float64 fold over the bin, times sum |rep|
    (every sample's fold error meeting a replica sample with the worst sign).  Loose on purpose:
    the structure of this path is held by the integer-exact tests."""
    fd = fold(iq, f, cs, n_coh)
    rep = np.abs(replica(prn, cs, reps))
    mag = np.abs(fd)      # (the two components' error sums are the legs of a triangle: Minkowski)
    prod = np.fft.ifft(np.fft.fft(mag) * np.conj(np.fft.fft(rep))).real
    e_fold = np.max(np.abs(oracle_fold(iq, f, cs, n_coh).astype(np.complex128) - fd)) * np.sum(rep)
    return cs * 2.0 ** -24 * prod + e_fold


# ---- integer-valued inputs at 0 Hz: the exact surface ------------------------------------------

def exact_integer_record(iq, prn, cs, n_coh, reps, surface=False):
    """For iq with integer real and imaginary parts, an integer replica, the bin 0 Hz (p = 0, the
    wipe-off factor exactly 1) and n_coh a power of two: n_coh times the correlation is an integer
    in both parts, so the float64 FFT correlation is rounded to the nearest multiple of 1 / n_coh
    before |.| and the surface is exact up to float64's own |.|."""
    x = _c64(iq)[:n_coh * cs].astype(np.complex128)
    rep = replica(prn, cs, reps)
    assert n_coh & (n_coh - 1) == 0
    assert np.array_equal(x.real, np.rint(x.real)) and np.array_equal(x.imag, np.rint(x.imag))
    assert np.array_equal(rep, np.rint(rep))
    total = x.reshape(n_coh, cs).sum(axis=0)                       # n_coh * fold, exact
    c = np.fft.ifft(np.fft.fft(total) * np.conj(np.fft.fft(rep)))
    assert max(np.max(np.abs(c.real - np.rint(c.real))), np.max(np.abs(c.imag - np.rint(c.imag)))) < 1e-6
    S = np.hypot(np.rint(c.real), np.rint(c.imag)) / n_coh
    return (record(S), S) if surface else record(S)


def integer_dot(iq, prn, cs, n_coh, reps, lag):
    """n_coh * sum_m fold[m] rep[(m - lag) mod cs] by integer dot products: (re, im) as Python ints."""
    x = _c64(iq)[:n_coh * cs]
    re = np.rint(x.real).astype(np.int64).reshape(n_coh, cs).sum(axis=0)
    im = np.rint(x.imag).astype(np.int64).reshape(n_coh, cs).sum(axis=0)
    r = np.roll(np.rint(replica(prn, cs, reps)).astype(np.int64), lag)     # r[m] = rep[m - lag]
    return int(np.dot(re, r)), int(np.dot(im, r))


# ---- deviations of a float32 realisation from the float64 records ------------------------------

METRICS = ('peak', 'lo', 'hi', 'mean', 'std')


def deviations(got, ref):
    """Per cell and field how far `got` (records with FIELDS) is from `ref`: peak, lo, hi and mean
    as |value - ref| / rms (lo and hi can be near zero: a relative error means nothing for them),
    std relatively.  0 on an all-zero reference surface where the value is 0 too."""
    d = {}
    for k in METRICS:
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        scale = ref['std'] if k == 'std' else ref['rms']
        with np.errstate(divide='ignore', invalid='ignore'):
            d[k] = np.where(err == 0, 0.0, err / scale)
    return d


# ---- the seeded inputs of test_gpu_acq_ref.py ---------------------------------------------------

BINS = (-5000.0, 5000.0, 0.0, -1250.0, 2500.0)
# deep cases: with carrier_hz = n_coh cs / K the shift of segment s is rint(-f K s); these bins give
# 0, a small one, cs - 1 and one far up at s = 1
DEEP_BINS = (-5000.0, 5000.0, 0.0, -25.0, 25.0)
# ... at 16368 one that crosses a layout row of 1023 lags (1101 = 1023 + 78) and one that carries
# into the next row for the upper threads (551); no shift of a few samples there: at 16 samples a
# chip the sum of two surfaces a fraction of a chip apart has a flat top, and flat tops are near ties
DEEP_BINS_16368 = (-5000.0, 5000.0, 0.0, -2500.0, 2500.0)
PRESENT = (1, 9, 20, 29, 37)
ABSENT = (4, 15)
PRNS = (1, 4, 9, 15, 20, 29, 37)
NOISE_SIGMA = 0.35


def peak_lags(cs, path):
    """The lags the present PRNs are put at, three to five per input, the last one the marginal
    replica's: 0, cs - 1 and both sides of the path's internal boundary; the 2048 path has two
    boundaries and therefore two inputs, 65536 one strong replica per input (case_inputs)."""
    if path == 'fft2048':                      # the 256-lane rows
        return ((0, 256, 1791, 1100), (2047, 255, 1792, 600))
    if path == 'pfa':                          # lag t + 1023 j: the layout rows
        return ((0, cs - 1, 1022, 1023, 7000),)
    if path == 'big':                          # n = 2048 n1 + n2: the n2 rows (255 / 256 below 2049)
        b = 2048 if cs > 2049 else 256
        return ((0, cs - 1, b - 1, b, cs // 2 + 3),)
    assert path == 'direct'                    # the 1024-lag tiles (cs 1024 has one: its last rows)
    if cs == 65536:                            # two PRNs are searched there: the two ends, one marginal
        return ((0, cs - 1, cs // 2 + 37),) * 2
    b = 1024 if cs > 1024 else 512
    return ((0, cs - 1, b - 1, b, cs // 2 + 37),)


def signal_input(cs, n_periods, lags, seed, weights=None):
    """complex64 [n_periods cs]: seeded Gaussian noise (sigma 0.35 per component) plus one rolled
    replica per lag, PRNs PRESENT in order, strong on the bins and (the last one) marginal between
    them.  weights: a factor per replica.  Returns (iq, [(prn, doppler, lag, amp, strong)]); a strong
    replica is expected at its lag."""
    rng = np.random.default_rng(seed)
    n = n_periods * cs
    x = NOISE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(1, n + 1, dtype=np.float64) / (1000.0 * cs)
    dopplers = (0.0, -5000.0, 5000.0, 2500.0, 625.0)
    # a sample is 1/16 (1/64) of a chip at 16 (65) Msps and the replica's edges are ramps: the peak
    # stands out of its neighbours by 1 % (0.06 %), so the replicas are that much stronger there
    k = 1 if cs <= 4096 else 5 if cs <= 16400 else 10
    amps = tuple(k * a for a in (0.12, 0.10, 0.10, 0.08, 0.05))
    sats = []
    for i, lag in enumerate(lags):
        prn, f, a = PRESENT[i], dopplers[i], amps[i]
        strong = True
        if i == len(lags) - 1:
            f, a, strong = dopplers[4], amps[4], False
        if weights is not None:
            a, strong = a * weights[i], strong and weights[i] == 1
        code = np.tile(np.roll(replica(prn, cs), lag), n_periods)
        x += a * code * np.exp(1j * (2 * np.pi * f * t + 0.7 * i))
        sats.append((prn, f, int(lag), a, strong))
    return x.astype(np.complex64), sats


def integer_replicas(cs, seed):
    """{prn: +-1 float32 vector [cs]} for PRNS: what the integer tests upload in place of GPSCacode."""
    rng = np.random.default_rng(seed)
    return {p: (2.0 * rng.integers(0, 2, cs) - 1.0).astype(np.float32) for p in PRNS}


def integer_lags(cs):
    """0, cs - 1, both sides of the first lag tile's end (cs 1024: of its rows), one mid-tile."""
    b = 1024 if cs > 1024 else 512
    return (0, cs - 1, b - 1, b, cs // 2 + 37)


def integer_input(cs, n_periods, reps, seed):
    """complex64 [n_periods cs] with real and imaginary parts drawn from -3 .. 3, plus a roll(rep, d)
    (a = 1, 2 alternating) for the PRESENT PRNs at integer_lags."""
    rng = np.random.default_rng(seed)
    n = n_periods * cs
    x = rng.integers(-3, 4, n).astype(np.float64) + 1j * rng.integers(-3, 4, n)
    sats = []
    for i, lag in enumerate(integer_lags(cs)):
        a = 1 + i % 2
        x += a * np.tile(np.roll(np.asarray(reps[PRESENT[i]], np.float64), lag), n_periods)
        sats.append((PRESENT[i], 0.0, int(lag), a))
    return x.astype(np.complex64), sats


def tie_lags(cs):
    """The last lag and the last lag of the first tile (cs 1024: of its first half): the first index
    must win, and it is the one that is not at the end."""
    return (cs - 1, (1024 if cs > 1024 else 512) - 1)


def tie_input(cs, n_periods, reps, prn, lags, a=2):
    """The same replica at two rolls with equal integer amplitude and no noise: the two peaks of the
    exact surface are the same integer."""
    r = np.asarray(reps[prn], np.float64)
    x = a * (np.roll(r, lags[0]) + np.roll(r, lags[1]))
    return np.tile(x, n_periods).astype(np.complex64)


# ---- the matrix of test_gpu_acq_ref.py -----------------------------------------------------------
# name: (path, code_samples, option "codephase" at handle creation, searches); a search is
# ('coh', n_avg) or ('nc' | 'deep', n_coh, n_seg).  Every row searches PRNS x BINS (DEEP_BINS for
# 'deep') unless CELLS says otherwise.
MATRIX = {
    'fft2048_g1': ('fft2048', 2048, 0, (('coh', 1), ('coh', 2), ('coh', 3))),
    'fft2048_g4': ('fft2048', 2048, 0, (('coh', 4), ('coh', 5), ('coh', 6), ('coh', 7), ('coh', 32))),
    'fft2048_seg': ('fft2048', 2048, 0, (('nc', 1, 1), ('nc', 1, 2), ('nc', 5, 3),
                                         ('deep', 1, 1), ('deep', 1, 2), ('deep', 5, 3))),
    'pfa16368': ('pfa', 16368, 0, (('coh', 1), ('coh', 3), ('coh', 8), ('nc', 2, 3), ('deep', 2, 3))),
    'big1024': ('big', 1024, 0, (('coh', 1), ('coh', 4))),
    'big1040': ('big', 1040, 0, (('coh', 1), ('coh', 3))),
    'big4096': ('big', 4096, 0, (('coh', 2),)),
    'big16384': ('big', 16384, 0, (('coh', 1),)),
    'big16368': ('big', 16368, 2, (('coh', 2),)),
    'direct1024': ('direct', 1024, 1, (('coh', 1),)),
    'direct1040': ('direct', 1040, 1, (('coh', 1), ('coh', 2))),
    'direct16368': ('direct', 16368, 1, (('coh', 1),)),
    'direct16400': ('direct', 16400, 0, (('coh', 1), ('coh', 4))),
    'direct65536': ('direct', 65536, 0, (('coh', 2),)),
}
CELLS = {'direct65536': ((1, 9), (0.0, -5000.0))}        # the upper bound of the ABI: 2 PRNs x 2 bins
# K of the deep cases: carrier_hz = n_coh cs / K, so that segment s of bin f is rotated by rint(-f K s)
DEEP_K = {2048: 0.04, 16368: 0.22026}


def case_periods(name):
    """(n_cyc, code periods of input) a row needs: n_cyc just large enough for its n_coh."""
    searches = MATRIX[name][3]
    return max(s[1] for s in searches), max(s[1] * (s[2] if len(s) > 2 else 1) for s in searches)


_INPUTS = {}
# chosen so that every row stays under its near-tie cap (test_acq_ref.py asserts it): about 0.2 % of
# noise-only cells have their two largest lags within 1e-4 of each other
# (at 16 samples a chip and more the surfaces are smooth and 2 - 3 % are)
SEEDS = {'fft2048_g1': 7100, 'fft2048_g4': 8110, 'fft2048_seg': 8120, 'pfa16368': 10130,
         'big1024': 7150, 'big1040': 8160, 'big4096': 7170, 'big16384': 11180, 'big16368': 12190,
         'direct1024': 7200, 'direct1040': 7210, 'direct16368': 7220, 'direct16400': 8230,
         'direct65536': 12240}


def case_inputs(name):
    """[(iq, sats)]: the row's seeded inputs (two at 2048, one elsewhere), memoised and read-only."""
    if name not in _INPUTS:
        path, cs = MATRIX[name][:2]
        seed = SEEDS[name]
        out = []
        for i, lags in enumerate(peak_lags(cs, path)):
            # 65536: a sample is 1/64 chip and the other strong replica's cross-correlation, as smooth
            # as the peak is flat, would move it: one strong replica per input
            w = None if cs != 65536 else ((1, 0.2, 1), (0.2, 1, 1))[i]
            iq, sats = signal_input(cs, case_periods(name)[1], lags, seed + i, w)
            iq.setflags(write=False)
            out.append((iq, sats))
        _INPUTS[name] = out
    return _INPUTS[name]


def case_search(name, search):
    """(prns, freqs, n_coh, n_seg, shifts or None, carrier_hz or None) of one search of a row."""
    cs = MATRIX[name][1]
    prns, bins = CELLS.get(name, (PRNS, BINS))
    kind, n_coh = search[:2]
    n_seg = search[2] if len(search) > 2 else 1
    if kind != 'deep':
        return list(prns), list(bins), n_coh, n_seg, None, None
    carrier = n_coh * cs / DEEP_K[cs]
    bins = DEEP_BINS if cs == 2048 else DEEP_BINS_16368
    return list(prns), list(bins), n_coh, n_seg, deep_shifts(bins, n_coh, n_seg, cs, carrier), carrier


_REFS = {}


def case_reference(name, search, which):
    """(records, near-tie surfaces) of one search on input `which` of a row in float64, memoised."""
    key = (name, search, which)
    if key not in _REFS:
        prns, freqs, n_coh, n_seg, shifts, _ = case_search(name, search)
        surf = {}
        rec = acq_ref(case_inputs(name)[which][0], freqs, prns, MATRIX[name][1], n_coh, n_seg, shifts,
                      surfaces=surf)
        rec.setflags(write=False)
        _REFS[key] = (rec, surf)
    return _REFS[key]


def excused_cap(ncells):
    """How many near-tie cells a test may leave out of the argmax equality: none below 100 cells,
    1 % otherwise."""
    return 0 if ncells < 100 else int(0.01 * ncells)


# ---- the second chunk of big_corr_launch: 37 PRNs x 14 bins = 518 cells at 1024 samples ----------
CHUNK_CS = 1024
CHUNK_PRNS = tuple(range(1, 38))
CHUNK_BINS = tuple(-3250.0 + 500.0 * i for i in range(14))


def chunk_input():
    return signal_input(CHUNK_CS, 1, peak_lags(CHUNK_CS, 'big')[0], 7300)[0]


# ---- the integer cases: the time-domain lengths of the matrix, and two of the 32768 pair -------
INTEGER_DIRECT = {name: row[1:3] for name, row in MATRIX.items() if row[0] == 'direct'}
INTEGER_BIG = (1040, 16384)
INTEGER_N_AVG = (1, 2, 4)


def integer_case(cs):
    """(reps, iq, sats, n_avgs) of a code length: n_cyc 4, or 2 at the ABI's upper bound."""
    key = ('int', cs)
    if key not in _INPUTS:
        n_avgs = tuple(n for n in INTEGER_N_AVG if n * cs <= 2 * 65536)
        reps = integer_replicas(cs, 8000 + cs)
        iq, sats = integer_input(cs, max(n_avgs), reps, 8001 + cs)
        iq.setflags(write=False)
        _INPUTS[key] = (reps, iq, sats, n_avgs)
    return _INPUTS[key]
