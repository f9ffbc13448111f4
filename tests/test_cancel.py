"""Strong-satellite cancellation (gpsmi_acq_cancel), the parts that need no GPU: the float64
restatement (cancel_ref.py) against the prototype the feature was specified with, and the ABI's
declarations, struct sizes, plan and argument errors.

Prototype, one amplitude-0.11 satellite, noise-free and unquantised, 64 ms, Dopplers +3094 and
-4321 Hz: the residual is -55 .. -59 dB with the true parameters, -45 dB with the frequency 3 Hz and
the code start 0.3 sample off, -35 dB at 10 Hz / 0.45 sample.  Asserted: -50, -40, -30 dB (5 dB of
margin each, for platform rounding).  On the collision scene (cancel_ref.collision_scene, PRN 3 at
amplitude 0.00772 two Hz from PRN 4 modulo 1 kHz) the largest peak of PRN 3 in the 1400 Hz bin is a
cross-correlation at delay 1157 with normMaxCorr 6.3 before and the satellite at 1200 with 18.8
after the three strong satellites are cancelled with parameters 2 Hz and 0.2 sample off."""
import ctypes as C

import numpy as np
import pytest

import cancel_ref as R


# ---- the restatement against the prototype --------------------------------------------------------

@pytest.mark.parametrize('doppler', R.DEPTH_DOPPLERS)
def test_residual_depth(doppler):
    x, tau, prn = R.depth_scene(doppler)
    for df, dt, bound in R.DEPTH_CASES:
        y, rec, coef, done = R.cancel_ref(x, [(prn, doppler + df, tau + dt)], 2048)
        db = R.residual_db(y, x)
        print('doppler %+6.0f  %4.1f Hz %4.2f sample off: residual %6.1f dB (bound %.0f)' % (doppler, df, dt, db, bound))
        assert rec['n_skipped'][0] == 0 and rec['n_windows'][0] == R.DEPTH_MS + 1
        assert db <= bound


def test_windows_tile_the_data():
    """Every sample belongs to exactly one window, whatever the sign of tau and of the Doppler."""
    for cs, n in ((2048, 5 * 2048 + 123), (16368, 130944)):
        for f in (-4321.0, 0.0, 3094.0):
            for tau in (-3000.7, -0.4, 0.0, 0.6, 5.5, 16.0, cs - 0.3, cs + 2.5):
                w = R.cancel_windows(n, cs, f, tau)
                assert w[0][0] == 0 and w[-1][1] == n
                assert all(a[1] == b[0] for a, b in zip(w, w[1:])) and all(hi > lo for lo, hi, _ in w)
                assert all(cs - 1 <= hi - lo <= cs + 1 for lo, hi, _ in w[1:-1])
                assert all(abs(j - lo) <= cs + 1 for lo, _, j in w)


@pytest.fixture(scope='module')
def collision():
    from gpsmi.synth import raw_to_c64
    x = raw_to_c64(R.collision_raw())
    sats = [(p, f + 2.0, R.true_tau(f, d) + 0.2) for p, f, d in R.COLLISION_STRONG]
    y, rec, _, _ = R.cancel_ref(x, sats, 2048)
    return x, y, rec


def test_collision_scene_peak_moves_to_the_satellite(collision):
    x, y, rec = collision
    before = R.norm_max_corr(R.nc_surface(x, 3, R.COLLISION_BIN))
    after = R.norm_max_corr(R.nc_surface(y, 3, R.COLLISION_BIN))
    print('PRN 3 in the 1400 Hz bin: %.2f @ %d before, %.2f @ %d after' % (*before, *after))
    assert before[0] < 8.0 and before[1] != 1200
    assert after[0] > 8.0 and after[1] == 1200
    absent = R.norm_max_corr(R.nc_surface(y, 10, R.COLLISION_BIN))[0]
    own = R.norm_max_corr(R.nc_surface(y, 4, 400.0))[0]
    drop = 10.0 * np.log10(np.sum(np.abs(y) ** 2) / np.sum(np.abs(x) ** 2))
    print('absent PRN 10 after %.2f, cancelled PRN 4 in its own bin %.2f, power %.2f dB' % (absent, own, drop))
    assert absent < 5.0 and own < 5.0
    assert np.all(rec['n_skipped'] == 0)
    ratio = rec['energy_removed'] / rec['energy_in']
    assert np.all((ratio > 0.02) & (ratio < 0.2))


# ---- ABI --------------------------------------------------------------------------------------------

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_struct_sizes():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(13) == C.sizeof(_lib.CancelSat) == _lib.CANCEL_SAT_DTYPE.itemsize == 24
    assert lib.gpsmi_abi_sizeof(14) == C.sizeof(_lib.CancelCfg) == 24
    assert lib.gpsmi_abi_sizeof(15) == C.sizeof(_lib.CancelOut) == _lib.CANCEL_OUT_DTYPE.itemsize == 32
    assert lib.gpsmi_abi_sizeof(16) == -1 and lib.gpsmi_abi_sizeof(99) == -1
    for dt, st in ((_lib.CANCEL_SAT_DTYPE, _lib.CancelSat), (_lib.CANCEL_OUT_DTYPE, _lib.CancelOut)):
        assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize       # no implicit padding
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    covered = sum(getattr(_lib.CancelCfg, n).size for n, _ in _lib.CancelCfg._fields_)
    assert covered == C.sizeof(_lib.CancelCfg)
    for name in ('gpsmi_acq_cancel', 'gpsmi_acq_cancel_dev', 'gpsmi_acq_cancel_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _plan(cs, n, sats, cfg=None):
    from gpsmi import _lib
    lib = _lib.load()
    s_a = np.zeros(len(sats), _lib.CANCEL_SAT_DTYPE)
    for i, (prn, f, tau) in enumerate(sats):
        s_a[i] = (prn, 0, f, tau)
    mw = C.c_int(-7)
    rc = lib.gpsmi_acq_cancel_plan(cs, n, _p(s_a), len(s_a), C.byref(cfg) if cfg is not None else None, C.byref(mw))
    return rc, mw.value, lib.gpsmi_last_error().decode()


def test_plan_counts_the_windows():
    for cs, n in ((2048, 5 * 2048 + 123), (16368, 130944)):
        sats = [(4, 3094.0, -0.4), (5, -4321.0, cs - 0.3), (9, 400.0, 5.5)]
        rc, mw, msg = _plan(cs, n, sats)
        assert rc == 0, msg
        assert mw == max(len(R.cancel_windows(n, cs, f, tau)) for _, f, tau in sats)
        for k in range(3):
            assert _plan(cs, n, sats[k:k + 1])[1] == len(R.cancel_windows(n, cs, *sats[k][1:]))
    assert _plan(2048, 1000, [])[:2] == (0, 0)                  # nsat = 0 is legal
    # f_offset and the carrier enter the code period
    from gpsmi import _lib
    cfg = _lib.CancelCfg(1575.42e6, 1.0e6, 0, 0)
    n = 3000 * 2048
    assert _plan(2048, n, [(4, 1.0e6, 0.0)], cfg)[1] == 3000
    assert _plan(2048, n, [(4, 1.0e6, 0.0)])[1] == 3002           # the code is 0.063 % shorter


def test_argument_errors_need_no_gpu():
    from gpsmi import _lib
    E_ARG, E_UNSUPPORTED = -1, -5
    ok = [(4, 3094.0, 17.5)]
    n = 5 * 2048
    assert _plan(2048, n, ok)[0] == 0
    def refused(code, reason, *args):              # (max_windows is left as it was)
        assert _plan(*args) == (code, -7, 'gpsmi_acq_cancel: ' + reason), (args, _plan(*args))
    refused(E_ARG, 'nsat out of range 0..32', 2048, n, ok * 33)   # nsat beyond 32 (and a PRN twice)
    refused(E_ARG, 'nsat out of range 0..32', 2048, n, [(p, 0.0, 0.0) for p in range(1, 34)])
    assert _plan(2048, n, [(p, 0.0, 0.0) for p in range(1, 33)])[0] == 0
    for bad, reason in (((0, 0.0, 0.0), 'prn out of range 1..37'), ((38, 0.0, 0.0), 'prn out of range 1..37'),
                        ((4, np.nan, 0.0), 'f_hz out of range'), ((4, np.inf, 0.0), 'f_hz out of range'),
                        ((4, 0.0, np.nan), 'tau out of range'), ((4, 0.0, -np.inf), 'tau out of range'),
                        ((4, 1.1e6, 0.0), 'f_hz out of range')):
        refused(E_ARG, reason, 2048, n, [bad])
    refused(E_ARG, 'a PRN appears twice', 2048, n, [(4, 0.0, 0.0), (5, 1.0, 2.0), (4, 3.0, 4.0)])
    refused(E_ARG, 'n out of range 1..2^40', 2048, 0, ok)
    refused(E_ARG, 'f_hz - f_offset_hz beyond 1 % of carrier_hz', 2048, n, [(4, 900000.0, 0.0)],
            _lib.CancelCfg(1.0e7, 0.0, 0, 0))
    for cs in (1024, 4096, 16384):
        refused(E_UNSUPPORTED, f'code_samples 2048 and 16368 only ({cs})', cs, n, ok)
    assert _plan(16368, n, ok)[0] == 0
    for cfg, reason in ((_lib.CancelCfg(-1.0, 0.0, 0, 0), 'carrier_hz must be positive (0: L1)'),
                        (_lib.CancelCfg(np.nan, 0.0, 0, 0), 'carrier_hz must be positive (0: L1)'),
                        (_lib.CancelCfg(0.0, np.inf, 0, 0), 'f_offset_hz must be finite'),
                        (_lib.CancelCfg(0.0, 0.0, -1, 0), 'min_window must be >= 1 (0: 16)')):
        refused(E_ARG, reason, 2048, n, ok, cfg)
    assert _plan(2048, n, ok, _lib.CancelCfg(0.0, 0.0, 0, 0))[0] == 0
    lib = _lib.load()
    assert lib.gpsmi_acq_cancel_plan(2048, n, None, 1, None, None) == E_ARG
    assert lib.gpsmi_last_error().decode() == 'gpsmi_acq_cancel: null argument'
    assert lib.gpsmi_acq_cancel_plan(2048, n, None, -1, None, None) == E_ARG
    assert lib.gpsmi_last_error().decode() == 'gpsmi_acq_cancel: nsat out of range 0..32'
