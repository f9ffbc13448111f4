"""Float64 numpy restatement of the code-phase correlation of tracking (trk_corr_kernel,
csrc/gpsmi_trk_corr.h; cacodeCorr + findCodePhase + fitCodePhase of the reference), shared by
test_corr_ref.py (CPU) and test_gpu_trk_corr.py (GPU).  Written from include/gpsmi.h and the
kernel's header comment; nothing of the oracle's float32 path is used.

For one block x (complex64 [N_CYC * 2048], or the recorder's uint16 decoded by the unpack formula)
and one state row (prn, freq, omega0, phase, delay), with fs = 1000 * 2048:
    om      = omega0 if it is non-zero, else float32(float32(2 pi) * freq): the float32 the
              kernel takes -- an input of the operation, not an error of it
    wiped   = x[k] exp(-j (phase + om (k + 1) / fs))
    fold    = mean of the centre n = min(CORR_AVG, N_CYC) code periods, from period (N_CYC - n) // 2
    corr    = |ifft(fft(fold) conj(fft(GPSCacode(prn))))|
    mx      = first-index argmax; epl = corr[mx - 1], corr[mx], corr[mx + 1] circularly
    norm    = (corr[mx] - mean) / population std
    delay, code_phase = mx, fitCodePhase when norm > CORR_MIN, else -1, -1.0
    delay_used = the forced delay if it is >= 0, else the found delay, else the state's
everything in float64 / complex128 with exact sample times."""
import numpy as np

CS = 2048
FS = 1000.0 * CS

CORR_DTYPE = np.dtype([
    ('mx', np.int32), ('epl', np.float64, (3,)), ('corr_mean', np.float64),
    ('corr_std', np.float64), ('norm_max_corr', np.float64), ('delay', np.int32),
    ('code_phase', np.float64), ('delay_used', np.int32),
    # what the tests scale by and what tells them that a discrete answer is not determined
    ('rms', np.float64),          # sqrt(mean(corr^2))
    ('gap', np.float64),          # (largest - second largest lag) / largest
    ('margin', np.float64)])      # |norm - CORR_MIN|

# the eight fields of a gpsmi_trk_out record that the code-phase correlation writes
FIELDS = ('mx', 'epl', 'corr_mean', 'corr_std', 'norm_max_corr', 'delay', 'code_phase', 'delay_used')

_SPEC = {}


def replica_spectrum(prn):
    """fft(GPSCacode(prn)) in float64 (the replica the engine is given, before its rounding to
    complex64)."""
    if prn not in _SPEC:
        from gpsmi import codes
        _SPEC[prn] = np.fft.fft(codes.code_replica(int(prn), CS))
    return _SPEC[prn]


def decode_u8(raw):
    """uint16 (Q << 8 | I) -> complex64, the unpack formula of gpsmi_dev_unpack_u8iq: each part
    float32(float32(byte) * float32(1 / 127.5)) - 1."""
    raw = np.asarray(raw, dtype=np.uint16)
    scl = np.float32(1.0) / np.float32(127.5)
    re = (raw & 0xFF).astype(np.float32) * scl - np.float32(1)
    im = (raw >> 8).astype(np.float32) * scl - np.float32(1)
    out = np.empty(raw.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def omega_f32(freq, omega0):
    """The float32 angular frequency the kernel wipes off with."""
    if np.float32(omega0) != 0:
        return np.float32(omega0)
    return np.float32(np.float32(2 * np.pi) * np.float32(freq))


def fit_code_phase(lo, pk, hi, mx):
    """fitCodePhase: the mean of a triangle and a parabola through the peak and its neighbours."""
    tri = 0.5 * (hi - lo) / (pk - (hi if lo > hi else lo))
    par = 0.5 * (hi - lo) / (2.0 * pk - hi - lo)
    return mx + 0.5 * (tri + par)


def corr_surface(block, prn, freq, omega0, phase, n_cyc, corr_avg):
    """float64 [2048]: the correlation magnitudes of one (block, channel) job."""
    x = np.asarray(block)
    if x.dtype == np.uint16:
        x = decode_u8(x)
    assert x.shape == (n_cyc * CS,)
    n = min(int(corr_avg), int(n_cyc))
    first = (n_cyc - n) // 2
    om = float(omega_f32(freq, omega0))
    k = np.arange(first * CS, (first + n) * CS, dtype=np.float64)
    arg = float(np.float32(phase)) + om * ((k + 1.0) / FS)
    wiped = x[first * CS:(first + n) * CS].astype(np.complex128) * np.exp(-1j * arg)
    fold = wiped.reshape(n, CS).sum(axis=0) / n
    return np.abs(np.fft.ifft(np.fft.fft(fold) * np.conj(replica_spectrum(prn))))


def corr_record(corr, corr_min, state_delay, forced=-1):
    """The CORR_DTYPE record of a correlation surface."""
    r = np.zeros((), CORR_DTYPE)
    mx = int(np.argmax(corr))
    n = len(corr)
    lo, pk, hi = corr[(mx - 1) % n], corr[mx], corr[(mx + 1) % n]
    mean, std = np.mean(corr), np.std(corr)
    norm = (pk - mean) / std
    r['mx'], r['epl'], r['corr_mean'], r['corr_std'], r['norm_max_corr'] = mx, (lo, pk, hi), mean, std, norm
    if norm > corr_min:
        r['delay'], r['code_phase'] = mx, fit_code_phase(lo, pk, hi, mx)
    else:
        r['delay'], r['code_phase'] = -1, -1.0
    used = int(r['delay']) if r['delay'] >= 0 else int(state_delay)
    if forced >= 0:
        used = int(forced)
    r['delay_used'] = used
    second = np.max(np.delete(corr, mx))
    r['rms'] = np.sqrt(np.mean(corr * corr))
    r['gap'] = (pk - second) / pk
    r['margin'] = abs(norm - corr_min)
    return r


def corr_ref(block, state, n_cyc, corr_avg, corr_min, forced=-1):
    """One job: block, one state row (any record with prn, freq, omega0, phase, delay), the
    configuration and the job's forced delay (-1: none) -> CORR_DTYPE record."""
    corr = corr_surface(block, int(state['prn']), state['freq'], state['omega0'], state['phase'],
                        n_cyc, corr_avg)
    return corr_record(corr, corr_min, int(state['delay']), int(forced))


def oracle_record(block, state, n_cyc, corr_avg, corr_min, forced=-1):
    """The same record from the project's float32 oracle (SatStream.cacode_corr behind
    demod_doppler, float32 carrier phase): what the tests measure their bounds with.  FREQ is a
    Python float where the state carries omega0 (float32(2 pi FREQ) of the float64 product) and a
    float32 where it does not, as in the oracle's own closed loop."""
    import gps_oracle as orc
    p = orc.Params(n_cyc=n_cyc, corr_avg=corr_avg, corr_min=corr_min)
    x = np.asarray(block)
    if x.dtype == np.uint16:
        x = decode_u8(x)
    if np.float32(state['omega0']) != 0:
        freq = float(np.float64(state['omega0']) / (2 * np.pi))
        assert np.float32(2 * np.pi * freq) == np.float32(state['omega0'])
    else:
        freq = np.float32(state['freq'])
    ss = _oracle_stream(int(state['prn']), p)
    wiped, _ = orc.demod_doppler(x, freq, np.float32(state['phase']), p.ngps, ss.t)
    corr, _, _, _ = ss.cacode_corr(wiped, ss.corr_avg)
    return corr_record(np.asarray(corr, np.float64), corr_min, int(state['delay']), int(forced))


_STREAMS = {}


def _oracle_stream(prn, p):
    import gps_oracle as orc
    key = (prn, p.n_cyc, p.corr_avg, p.corr_min)
    if key not in _STREAMS:
        _STREAMS[key] = orc.SatStream(prn, 0.0, p)
    return _STREAMS[key]


# ---- deviations of a float32 realisation (the oracle, the kernel) from the float64 records

METRICS = ('epl', 'corr_mean', 'corr_std', 'norm_max_corr', 'code_phase')


def deviations(got, ref):
    """Per job and field, how far `got` (any records with FIELDS) is from the float64 records
    `ref`: epl / corr_mean / corr_std as absolute errors over the float64 surface's rms,
    norm_max_corr relatively, code_phase absolutely in samples (0 where either side has no fit).
    Returns a dict of float64 arrays shaped like ref."""
    got_epl = np.asarray(got['epl'], np.float64)
    d = {'epl': np.max(np.abs(got_epl - ref['epl']), axis=-1) / ref['rms'],
         'corr_mean': np.abs(np.asarray(got['corr_mean'], np.float64) - ref['corr_mean']) / ref['rms'],
         'corr_std': np.abs(np.asarray(got['corr_std'], np.float64) - ref['corr_std']) / ref['rms'],
         'norm_max_corr': np.abs(np.asarray(got['norm_max_corr'], np.float64) - ref['norm_max_corr'])
         / np.abs(ref['norm_max_corr'])}
    both = (np.asarray(got['delay']) >= 0) & (ref['delay'] >= 0)
    d['code_phase'] = np.where(both, np.abs(np.asarray(got['code_phase'], np.float64) - ref['code_phase']), 0.0)
    return d
