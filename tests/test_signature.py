"""Spatial signatures without a GPU: the argument checks of
gpsmi_acq_signature_plan, the struct layouts, the float64 restatement (sig_ref.py) on scenes whose
answer is known, and the host decision (snapshot.signature_vectors / signature_rho / spoof_resolve)
on hand-made covariances."""
import ctypes as C

import numpy as np
import pytest

import sig_ref as R
from gpsmi import _lib, engine, snapshot as S

N = R.KERNEL_N[2048]
GOOD = [(4, 3096.0, 0.3), (5, -4319.0, 2047.7)]


def test_struct_sizes():
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(27) == _lib.SIG_SAT_DTYPE.itemsize == 24
    assert lib.gpsmi_abi_sizeof(28) == C.sizeof(_lib.SigCfg) == 24
    assert sum(_lib.SIG_SAT_DTYPE.fields[n][0].itemsize for n in _lib.SIG_SAT_DTYPE.names) == 24


def test_plan_counts_the_windows():
    for cs in (2048, 16368):
        n = R.KERNEL_N[cs]
        for n_ms in (0, 3):
            n_win, max_w = engine.signature_plan(cs, n, R.kernel_records(cs), 3, n_ms=n_ms)
            want = [len(R.sig_windows(n, cs, f, tau, n_ms)) for _, f, tau in R.kernel_records(cs)]
            assert n_win.tolist() == want and max_w == max(want)
    n_win, _ = engine.signature_plan(2048, N, R.kernel_records(2048), 2)
    assert n_win.tolist() == [6, 6, 5, 5]             # tau 0.3 and cs - 0.3 (k = -1: rint(-0.31) = 0): j = 0 is a window
    # the window rule is cancellation's: the same j wherever both have a whole window
    from cancel_ref import cancel_windows
    for _, f, tau in R.kernel_records(2048):
        whole = [j for lo, hi, j in cancel_windows(N, 2048, f, tau) if j >= 0 and j + 2048 <= N]
        assert R.sig_windows(N, 2048, f, tau) == whole


def test_a_repeated_prn_is_accepted():
    n_win, _ = engine.signature_plan(2048, N, [(4, 3096.0, 0.3), (4, 3091.0, 700.2), (4, 3096.0, 0.3)], 4)
    assert n_win.tolist() == [6, 5, 6]


def raw_plan(cs, n, sats, cfg, reserved=0, null_sats=False):
    lib = _lib.load()
    s_a = np.zeros(len(sats), _lib.SIG_SAT_DTYPE)
    for i, (p, f, t) in enumerate(sats):
        s_a[i] = (p, reserved, f, t)
    rc = lib.gpsmi_acq_signature_plan(cs, n, None if null_sats else _lib.ptr(s_a), len(sats),
                                      None if cfg is None else C.byref(cfg), None, None)
    return rc, lib.gpsmi_last_error().decode()


def cfg(A=4, n_ms=0, carrier=0.0, f_offset=0.0):
    return _lib.SigCfg(A, n_ms, carrier, f_offset)


def test_plan_accepts_defaults():
    assert raw_plan(2048, N, GOOD, None)[0] == 0      # cfg null: two antennas, every window, L1
    assert raw_plan(2048, N, GOOD, cfg(0))[0] == 0
    assert raw_plan(16368, R.KERNEL_N[16368], GOOD, cfg(8))[0] == 0


# the whole text behind "gpsmi_acq_signature: " of the refusal that holds the word
REASON = {'null': 'null argument', 'antennas': 'antennas out of range 2..8 (0: 2)', 'nsat': 'nsat out of range 1..64',
          'prn': 'prn out of range 1..37', 'f_hz': 'f_hz out of range', 'tau': 'tau out of range',
          '1 %': 'f_hz - f_offset_hz beyond 1 % of carrier_hz', 'n out of range': 'n out of range 1..2^40 / antennas',
          'reserved': 'a reserved field is not 0', 'n_ms': 'n_ms must be >= 1 (0: every window that fits)',
          'no window': 'a record has no window inside iq'}


@pytest.mark.parametrize('name,call,word', [
    ('null sats', lambda: raw_plan(2048, N, GOOD, cfg(), null_sats=True), 'null'),
    ('one antenna', lambda: raw_plan(2048, N, GOOD, cfg(1)), 'antennas'),
    ('nine antennas', lambda: raw_plan(2048, N, GOOD, cfg(9)), 'antennas'),
    ('negative antennas', lambda: raw_plan(2048, N, GOOD, cfg(-2)), 'antennas'),
    ('no record', lambda: raw_plan(2048, N, [], cfg()), 'nsat'),
    ('65 records', lambda: raw_plan(2048, N, GOOD[:1] * 65, cfg()), 'nsat'),
    ('prn 0', lambda: raw_plan(2048, N, [(0, 0.0, 0.0)], cfg()), 'prn'),
    ('prn 38', lambda: raw_plan(2048, N, [(38, 0.0, 0.0)], cfg()), 'prn'),
    ('f nan', lambda: raw_plan(2048, N, [(4, np.nan, 0.0)], cfg()), 'f_hz'),
    ('f inf', lambda: raw_plan(2048, N, [(4, np.inf, 0.0)], cfg()), 'f_hz'),
    ('tau nan', lambda: raw_plan(2048, N, [(4, 0.0, np.nan)], cfg()), 'tau'),
    ('tau inf', lambda: raw_plan(2048, N, [(4, 0.0, -np.inf)], cfg()), 'tau'),
    ('f at fs / 2', lambda: raw_plan(2048, N, [(4, 1024000.0, 0.0)], cfg()), 'f_hz'),
    ('f at -fs / 2', lambda: raw_plan(2048, N, [(4, -1024000.0, 0.0)], cfg()), 'f_hz'),
    ('beyond 1 % of the carrier', lambda: raw_plan(2048, N, [(4, 5000.0, 0.0)], cfg(carrier=4.0e5)), '1 %'),
    ('beyond 1 % by the offset', lambda: raw_plan(2048, N, [(4, 0.0, 0.0)], cfg(f_offset=-1.6e7)), '1 %'),
    ('n 0', lambda: raw_plan(2048, 0, GOOD, cfg()), 'n out of range'),
    ('n beyond 2^40 / A', lambda: raw_plan(2048, (1 << 40) // 4 + 1, GOOD, cfg(4)), 'n out of range'),
    ('reserved', lambda: raw_plan(2048, N, GOOD, cfg(), reserved=1), 'reserved'),
    ('negative n_ms', lambda: raw_plan(2048, N, GOOD, cfg(n_ms=-1)), 'n_ms'),
    ('no window', lambda: raw_plan(2048, 2047, GOOD, cfg()), 'no window'),
], ids=lambda v: v if isinstance(v, str) else '')
def test_plan_argument_errors(name, call, word):
    rc, msg = call()
    assert rc == -1 and msg == 'gpsmi_acq_signature: ' + REASON[word], (name, rc, msg)


def test_plan_unsupported_code_length():
    rc, msg = raw_plan(4096, N, GOOD, cfg())
    assert rc == -5 and msg == 'gpsmi_acq_signature: code_samples 2048 and 16368 only (4096)'
    with pytest.raises(engine.EngineError):
        engine.signature_plan(2048, N, [(4, np.nan, 0.0)], 4)


def test_n_at_the_limit_is_taken():
    """n = 2^40 / A passes the range check (n_ms keeps the plan to one window)."""
    assert raw_plan(2048, (1 << 40) // 8, [(4, 0.0, 0.0)], cfg(8, n_ms=1))[0] == 0


# ---- the restatement ------------------------------------------------------------------------------
def test_identical_rows_give_an_equal_real_covariance():
    x = R.kernel_c64(2048)[0]
    P, Cv, n_win = R.sig_ref(np.stack([x, x, x]), R.kernel_records(2048), 2048)
    assert n_win.tolist() == [6, 6, 5, 5]
    for r in range(len(Cv)):
        assert np.array_equal(P[r, 0], P[r, 1]) and np.array_equal(P[r, 0], P[r, 2])
        assert np.all(Cv[r] == Cv[r, 0, 0]) and np.all(Cv[r].imag == 0) and Cv[r, 0, 0].real > 0
        assert np.all(P[r, :, n_win[r]:] == 0)
    v, q = S.signature_vectors(Cv)
    np.testing.assert_allclose(v, np.full((4, 3), 1.0 / np.sqrt(3.0)), atol=1e-12)
    assert np.all(S.signature_rho(v) > 1.0 - 1e-12)


# |v^H a| of the signature against the true steering vector a / |a| in the noise-free scene below,
# 20 ms: measured 1 - 3.77e-06, 1 - 2.10e-06 and 1 - 3.65e-08 (the other satellites' cross-correlation,
# 24 dB down and averaged over the windows, is what is left); asserted with ten times the largest deviation
STEERING_MIN = 1.0 - 10 * 3.77e-6


def test_noise_free_scene_gives_the_steering_vectors():
    from gpsmi import synth, synth_array
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=0.11, phase0=0.7 * i)
            for i, (p, f, d) in enumerate([(4, 3094.0, 15.7), (5, -4321.0, 900.4), (9, 400.0, 1347.4)])]
    sc = synth.Scene(sats=sats, seed=3, noise_sigma=0.0, code_samples=2048)
    steer = synth_array.ula_steering(4, [-0.6, 0.1, 0.75])
    x = synth_array.ArrayScene(sc, steer).block_float(0, n=20 * 2048 + 100)
    recs = [(s.prn, s.doppler, s.delay / (1.0 + s.doppler / R.L1_HZ)) for s in sats]
    _, Cv, n_win = R.sig_ref(x, recs, 2048)
    assert n_win.tolist() == [20, 19, 19]
    v, q = S.signature_vectors(Cv)
    for s in range(3):
        a = steer[:, s] / np.linalg.norm(steer[:, s])
        got = abs(np.vdot(a, v[s]))
        print('satellite %d: |v^H a| = 1 - %.2e, quality %.1f' % (s, 1.0 - got, q[s]))
        assert got >= STEERING_MIN and v[s, 0].imag == 0 and v[s, 0].real > 0
    rho = S.signature_rho(v)
    want = np.abs(steer.conj().T @ steer) / 4.0
    np.testing.assert_allclose(rho, want, atol=0.01)


# ---- the decision on hand-made covariances -------------------------------------------------------
def cov_of(sine, A=4, noise=0.01):
    a = np.exp(2j * np.pi * 0.5 * np.arange(A) * sine)
    return np.outer(a, a.conj()) + noise * np.eye(A)


def meas_of(prns):
    m = np.zeros(len(prns), S.MEAS_DTYPE)
    m['prn'], m['cn0_dbhz'] = prns, 45.0
    return m


def resolved(prns, sines, sets, doubled):
    rep = S.SpoofReport(doubled=list(doubled), alarm=len(doubled) >= S.SPOOF_MIN_DOUBLED)
    v, q = S.signature_vectors(np.stack([cov_of(s) for s in sines]))
    assert np.all(q > 100.0) and np.allclose(np.linalg.norm(v, axis=1), 1.0) and np.all(v[:, 0].imag == 0)
    return S.spoof_resolve(rep, meas_of(prns), sets, v), rep


def test_signature_vectors_and_rho():
    v, q = S.signature_vectors(np.stack([cov_of(0.3), cov_of(0.3, noise=0.5), cov_of(-0.5)]))
    a = np.exp(2j * np.pi * 0.5 * np.arange(4) * 0.3) / 2.0
    np.testing.assert_allclose(v[0], a, atol=1e-12)
    np.testing.assert_allclose(q, [4.01 / 0.01, 4.5 / 0.5, 4.01 / 0.01], rtol=1e-9)
    rho = S.signature_rho(v)
    assert rho.shape == (3, 3) and np.allclose(np.diag(rho), 1.0) and np.allclose(rho, rho.T)
    assert rho[0, 1] > 1.0 - 1e-12 and abs(rho[0, 2] - abs(np.sum(np.exp(2j * np.pi * 0.5 * np.arange(4) * 0.8))) / 4.0) < 1e-12


PRNS = [2, 2, 5, 5, 8, 8, 9]
SETS = ([0, 2, 4, 6], [1, 3, 5, 6])


def test_verdict():
    # set b's doubled records all arrive from the sine 0.3, set a's from all over the sky
    auth, rep = resolved(PRNS, [-0.8, 0.3, -0.2, 0.3, 0.6, 0.3, 0.1], SETS, [2, 5, 8])
    assert auth == 0 and rep.authentic == 0 and rep.one_source == (False, True) and not rep.one_direction
    auth, rep = resolved(PRNS, [0.3, -0.8, 0.3, -0.2, 0.3, 0.6, 0.1], SETS, [2, 5, 8])
    assert auth == 1 and rep.one_source == (True, False) and rep.alarm
    assert rep.rho.shape == (7, 7) and rep.signature.shape == (7, 4)


def test_no_verdict_when_both_sets_are_one_source():
    auth, rep = resolved(PRNS, [0.3, -0.5, 0.3, -0.5, 0.3, -0.5, 0.1], SETS, [2, 5, 8])
    assert auth is None and rep.authentic is None and rep.one_source == (True, True) and not rep.one_direction


def test_no_verdict_when_neither_is():
    auth, rep = resolved(PRNS, [0.3, -0.8, -0.2, 0.3, 0.3, 0.6, 0.1], SETS, [2, 5, 8])
    assert auth is None and rep.one_source == (False, False)
    # without a pair of fixes there are no sets to judge
    auth, rep = resolved(PRNS, [0.3, -0.8, 0.3, -0.2, 0.3, 0.6, 0.1], None, [2, 5, 8])
    assert auth is None and rep.one_source == (False, False)


def test_fewer_than_two_doubled_prns():
    """One doubled PRN leaves one doubled record per set: nothing to compare, no verdict -- the single
    records, which are in both sets, do not count."""
    auth, rep = resolved([2, 2, 5, 8, 9], [0.3, -0.8, 0.3, 0.3, 0.3], ([0, 2, 3, 4], [1, 2, 3, 4]), [2])
    assert auth is None and rep.one_source == (False, False) and not rep.alarm and not rep.one_direction


def test_one_direction():
    auth, rep = resolved([2, 5, 8, 9], [0.3] * 4, None, [])
    assert auth is None and rep.one_direction and rep.alarm and rep.doubled == []
    _, rep = resolved([2, 5, 8], [0.3] * 3, None, [])                  # three PRNs are too few
    assert not rep.one_direction and not rep.alarm
    _, rep = resolved([2, 5, 8, 9], [0.3, 0.3, 0.3, -0.4], None, [])   # one of them from elsewhere
    assert not rep.one_direction and not rep.alarm
    _, rep = resolved([2, 2, 5, 8, 9], [0.3] * 5, ([0, 2, 3, 4], [1, 2, 3, 4]), [2])   # twins included
    assert rep.one_direction and rep.alarm
    assert S.SPOOF_RHO_MIN == 0.95
