"""Float64 numpy restatement of the array search (gpsmi_acq_search_array, include/gpsmi.h; kernel:
csrc/gpsmi_acq_array.h), shared by test_acq_array.py (CPU) and test_gpu_acq_array.py (GPU).  Written
from include/gpsmi.h on acq_ref.py's phase argument, fold and replica; nothing float32 enters it but
the three float32 inputs of the operation (acq_ref.py's docstring).

For rows iq [A][n] (complex64, or the recorder's uint16 decoded), bins f, PRNs and (n_coh, n_seg,
shifts m [nbins][n_seg] in 0 .. cs - 1):
    c[a][s][n] = sum_k fold_{a,s}[k] rep[(k - n) mod cs]               (complex128, NOT its magnitude)
    D[i]       = sum_s sum_a |c[a][s][(i + m) mod cs]|^2
    R_ab[i]    = sum_s c[a][s][(i + m) mod cs] conj(c[b][s][(i + m) mod cs])            (a < b)
    T[i]       = (D[i] + 2 sum_{a<b} |R_ab[i]|) / (A n_seg)
    record     = acq_ref.record(T)

Beside it array_f32: the same in float32 on gps_oracle's float32 functions with the stated sum
order (ascending s, then ascending a, then the pairs in lexicographic order).  It is used to
measure bounds only: how far a float32 realisation of the operation is from the float64 one.

And the seeded inputs and cases of test_gpu_acq_array.py, so that the CPU file can hold them to
"no near tie in float64" without a GPU."""
import numpy as np

import acq_ref as ar

CS = 2048


def _rows(iq):
    x = np.asarray(iq)
    assert x.ndim == 2 and 2 <= x.shape[0] <= 4, x.shape
    return [ar._c64(r) for r in x]


def pairs(A):
    """(a, b), a < b, in lexicographic order."""
    return [(a, b) for a in range(A) for b in range(a + 1, A)]


# ---- the operation in float64 ----------------------------------------------------------------

def correlations(rows, f, prns, n_coh, n_seg, m=None, cs=CS, reps=None):
    """{prn: c complex128 [A, n_seg, cs]} of one bin: c[a][s][(i + m[s]) mod cs] at i, the segments
    already rotated.  rows: the antennas' samples, m: the bin's shifts [n_seg] or None."""
    fspec = np.array([[np.fft.fft(ar.fold(r, f, cs, n_coh, s)) for s in range(n_seg)] for r in rows])
    out = {}
    for p in prns:
        c = np.fft.ifft(fspec * np.conj(np.fft.fft(ar.replica(p, cs, reps))), axis=-1)
        if m is not None:
            for s in range(n_seg):
                if int(m[s]) % cs:
                    c[:, s] = np.roll(c[:, s], -int(m[s]), axis=-1)
        out[p] = c
    return out


def combine(c):
    """T float64 [cs] of one cell's rotated correlations c [A, n_seg, cs]."""
    A, n_seg = c.shape[:2]
    D = np.zeros(c.shape[-1])
    for s in range(n_seg):
        for a in range(A):
            D += np.abs(c[a, s]) ** 2
    cross = sum(np.abs(np.sum(c[a] * np.conj(c[b]), axis=0)) for a, b in pairs(A))
    return (D + 2.0 * cross) / (A * n_seg)


def array_surfaces(iq, freqs, prns, n_coh, n_seg, shifts=None, cs=CS, reps=None):
    """T, float64 [nbins, nsv, cs]."""
    rows = _rows(iq)
    out = np.zeros((len(freqs), len(prns), cs))
    for b, f in enumerate(freqs):
        c = correlations(rows, f, prns, n_coh, n_seg, None if shifts is None else shifts[b], cs, reps)
        for j, p in enumerate(prns):
            out[b, j] = combine(c[p])
    return out


def records(T):
    """REC_DTYPE [nbins, nsv] of surfaces [nbins, nsv, cs]."""
    out = np.zeros(T.shape[:2], ar.REC_DTYPE)
    for idx in np.ndindex(out.shape):
        out[idx] = ar.record(T[idx])
    return out


# ---- the same in float32, in the order gpsmi.h states ---------------------------------------------

def array_f32(iq, freqs, prns, n_coh, n_seg, shifts=None, cs=CS, reps=None):
    """T, float32 [nbins, nsv, cs]: gps_oracle's float32 wipe-off, folded spectrum and inverse
    transform (the replica spectrum complex64, as a handle holds it), float32 accumulators."""
    import gps_oracle as orc
    rows = _rows(iq)
    A = len(rows)
    t = ar.time_base(cs, n_coh * cs)
    rspec = [np.conjugate(ar._oracle_replica_spectrum(p, cs, reps)) for p in prns]
    out = np.zeros((len(freqs), len(prns), cs), np.float32)
    two, sc = np.float32(2.0), np.float32(1.0 / (A * n_seg))
    for b, f in enumerate(freqs):
        fspec = [[orc.folded_spectrum(ar._oracle_wiped(r, f, cs, n_coh, s, t), 0, n_coh, cs)
                  for s in range(n_seg)] for r in rows]
        for j in range(len(prns)):
            D = np.zeros(cs, np.float32)
            Rre = {p: np.zeros(cs, np.float32) for p in pairs(A)}
            Rim = {p: np.zeros(cs, np.float32) for p in pairs(A)}
            for s in range(n_seg):
                m = 0 if shifts is None else int(shifts[b][s])
                c = []
                for a in range(A):
                    ca = orc.ifft(fspec[a][s] * rspec[j])
                    assert ca.dtype == np.complex64
                    c.append(np.roll(ca, -m))
                for a in range(A):
                    D = D + (c[a].real * c[a].real + c[a].imag * c[a].imag)
                for (a, a2) in pairs(A):
                    Rre[(a, a2)] = Rre[(a, a2)] + (c[a].real * c[a2].real + c[a].imag * c[a2].imag)
                    Rim[(a, a2)] = Rim[(a, a2)] + (c[a].imag * c[a2].real - c[a].real * c[a2].imag)
            cross = np.zeros(cs, np.float32)
            for p in pairs(A):
                cross = cross + np.sqrt(Rre[p] * Rre[p] + Rim[p] * Rim[p])
            T = (D + two * cross) * sc
            assert T.dtype == np.float32
            out[b, j] = T
    return out


def records_f32(T32):
    """records() of float32 surfaces with mean and std formed in float32 (numpy's own order)."""
    out = records(T32.astype(np.float64))
    for idx in np.ndindex(out.shape):
        out[idx]['mean'], out[idx]['std'] = np.mean(T32[idx]), np.std(T32[idx])
    return out


def row_deviation(got, ref):
    """max over the lags of |got - ref| / rms(ref), per cell: [nbins, nsv]."""
    ref = np.asarray(ref, np.float64)
    rms = np.sqrt(np.mean(ref * ref, axis=-1))
    return np.max(np.abs(np.asarray(got, np.float64) - ref), axis=-1) / rms


# ---- the seeded inputs and cases of test_gpu_acq_array.py -----------------------------------------
# carrier_hz = n_coh cs / K makes the shift of segment s of bin f rint(-f K s) (acq_ref.DEEP_K): with
# K = 0.04 the bins below give m = 0 (0 Hz); 2047, 2046, .. (the rotated read wraps from its first
# lag on); and rint(1.5 s) = 2, 3, 4, 6 with its two ties to even.
K = ar.DEEP_K[CS]
BINS = (0.0, 25.0, -37.5)
PRNS = (9, 4, 20)                           # 9 and 20 are in the rows, 4 is not
ANTENNAS = (2, 3, 4)
SHAPES = ((1, 1), (1, 2), (1, 5), (4, 1), (4, 2), (4, 5))          # (n_coh, n_seg)
PLANTED = ((9, 0.0, 2047), (20, 25.0, 256))                        # (prn, doppler, lag)
AMP = 0.10
PHASES = (0.3, 2.1, 4.4, 5.5)                                      # per antenna, radians
SEED = 9200


def carrier(n_coh):
    return n_coh * CS / K


def shifts(n_coh, n_seg, freqs=BINS):
    return ar.deep_shifts(freqs, n_coh, n_seg, CS, carrier(n_coh))


_MEMO = {}


def planted_rows(A, n_periods, seed=SEED, planted=PLANTED):
    """(raw uint16 [A][n], its complex64 decode): seeded Gaussian noise (sigma 0.35 per component)
    plus the PLANTED replicas, antenna a's copy turned by PHASES[a] (and a further 0.9 a per
    replica, so that the two signatures differ), quantised as the recorder does.  Memoised,
    read-only."""
    key = ('rows', A, n_periods, seed, planted)
    if key not in _MEMO:
        rng = np.random.default_rng(seed + 10 * A)
        n = n_periods * CS
        tt = np.arange(1, n + 1, dtype=np.float64) / (1000.0 * CS)
        x = ar.NOISE_SIGMA * (rng.standard_normal((A, n)) + 1j * rng.standard_normal((A, n)))
        for i, (prn, f, lag) in enumerate(planted):
            code = np.tile(np.roll(ar.replica(prn, CS), lag), n_periods)
            for a in range(A):
                x[a] += AMP * code * np.exp(1j * (2 * np.pi * f * tt + PHASES[a] + 0.9 * a * i))
        q = lambda v: np.clip(np.rint((v + 1.0) * 127.5), 0, 255).astype(np.uint16)
        raw = np.ascontiguousarray((q(x.imag) << 8) | q(x.real))
        c64 = np.ascontiguousarray(np.stack([ar.decode_u8(r) for r in raw]))
        assert c64.dtype == np.complex64
        raw.setflags(write=False)
        c64.setflags(write=False)
        _MEMO[key] = (raw, c64)
    return _MEMO[key]


def case_rows(A, n_coh, n_seg):
    """The first n_seg n_coh periods of the A-antenna input (every shape reads the same rows)."""
    raw, c64 = planted_rows(A, max(c * s for c, s in SHAPES))
    n = n_coh * n_seg * CS
    return np.ascontiguousarray(raw[:, :n]), np.ascontiguousarray(c64[:, :n])


def case_reference(A, n_coh, n_seg):
    """(T float64 [3, 3, cs], its records, T of array_f32, its records) of a case, memoised."""
    key = ('ref', A, n_coh, n_seg)
    if key not in _MEMO:
        c64 = case_rows(A, n_coh, n_seg)[1]
        m = shifts(n_coh, n_seg)
        T = array_surfaces(c64, BINS, PRNS, n_coh, n_seg, m)
        T32 = array_f32(c64, BINS, PRNS, n_coh, n_seg, m)
        for a in (T, T32):
            a.setflags(write=False)
        _MEMO[key] = (T, records(T), T32, records_f32(T32))
    return _MEMO[key]


# ---- a call whose bins take two launches: 512 segments over two antennas are 16 MiB of spectra a
# bin, 32 bins a launch; bins 32 and 33 go into a second one --------------------------------------
CHUNK_A, CHUNK_N_COH, CHUNK_N_SEG = 2, 1, 512
CHUNK_BINS = tuple(-3300.0 + 200.0 * i for i in range(34))
CHUNK_PRNS = (9, 4)
CHUNK_OFFSET = 2.0e4                        # (test_gpu_acq_parent.py's: every bin slides, each its own way)


def chunk_rows():
    return planted_rows(CHUNK_A, CHUNK_N_COH * CHUNK_N_SEG, SEED + 1, ((9, -3300.0 + 200.0 * 33, 700),))


def chunk_reference():
    """(T float64 [1, 2, cs], its records, T of array_f32, its records) of the LAST bin, memoised.
    The planted code has no code Doppler while the search slides by up to 11 lags over the 512
    segments: its peak is a ridge over lags 689 .. 700, 46 or 47 segments a lag."""
    if 'chunk' not in _MEMO:
        c64 = chunk_rows()[1]
        bins = CHUNK_BINS[-1:]
        m = ar.deep_shifts(bins, CHUNK_N_COH, CHUNK_N_SEG, CS, f_offset=CHUNK_OFFSET)
        T = array_surfaces(c64, bins, CHUNK_PRNS, CHUNK_N_COH, CHUNK_N_SEG, m)
        T32 = array_f32(c64, bins, CHUNK_PRNS, CHUNK_N_COH, CHUNK_N_SEG, m)
        _MEMO['chunk'] = (T, records(T), T32, records_f32(T32))
    return _MEMO['chunk']
