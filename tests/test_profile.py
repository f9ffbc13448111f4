"""The multi-tap correlation profiles without a GPU: the ABI's layout and every
refusal of gpsmi_acq_profile_plan, its run counts against the restatement (profile_ref.py), the
properties of the restatement, snapshot.profile_fit on constructed covariances, and the restated chain
-- test_snapshot_spoof.py's chain, then profile_ref on its records, then snapshot.profile_verdict -- on
the clean second, the 30-us spoofed second and the lift-off second (liftoff_truth.py), which is where
PROFILE_T_MIN is measured."""
import copy
import ctypes as C

import numpy as np
import pytest

import liftoff_truth as LT
import profile_ref as R
import snapshot_truth as T
import spoof_truth as ST
from gpsmi import _lib, engine, snapshot as S, synth
from gpsmi.acquisition import profile_sats


# ---------------------------------------------------------------- the ABI and the plan
def test_abi_layout():
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(29) == _lib.PROF_SAT_DTYPE.itemsize == 24
    assert lib.gpsmi_abi_sizeof(30) == C.sizeof(_lib.ProfCfg) == 32
    assert lib.gpsmi_abi_sizeof(31) == -1
    assert sum(_lib.PROF_SAT_DTYPE.fields[n][0].itemsize for n in _lib.PROF_SAT_DTYPE.names) == 24
    assert sum(getattr(_lib.ProfCfg, n).size for n, _ in _lib.ProfCfg._fields_) == 32
    for name in ('gpsmi_acq_profile', 'gpsmi_acq_profile_dev', 'gpsmi_acq_profile_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _plan_rc(cs, n, sats, cfg):
    s_a = np.zeros(len(sats), _lib.PROF_SAT_DTYPE)
    for i, s in enumerate(sats):
        s_a[i] = s
    lib = _lib.load()
    return lib.gpsmi_acq_profile_plan(cs, n, _lib.ptr(s_a), len(s_a), None if cfg is None else C.byref(cfg),
                                      None, None, None), lib.gpsmi_last_error().decode()


def test_plan_refuses():
    n, ok = 45 * 2048, [(4, 0, 1000.0, 10.5)]
    cfg = lambda **k: _lib.ProfCfg(**{**dict(half_taps=0, coh_ms=0, n_runs=0, reserved=0, carrier_hz=0.0, f_offset_hz=0.0), **k})
    assert _plan_rc(2048, n, ok, None)[0] == 0 and _plan_rc(2048, n, ok, cfg())[0] == 0
    nan, inf = float('nan'), float('inf')
    bad = [('nsat', [], None), ('nsat', ok * 65, None), ('prn', [(0, 0, 0.0, 0.0)], None), ('prn', [(38, 0, 0.0, 0.0)], None),
           ('skip_ms', [(4, -1, 0.0, 0.0)], None), ('skip_ms', [(4, 20, 0.0, 0.0)], None),
           ('f_hz', [(4, 0, nan, 0.0)], None), ('f_hz', [(4, 0, 1024000.0, 0.0)], None), ('tau', [(4, 0, 0.0, inf)], None),
           ('tau', [(4, 0, 0.0, nan)], None), ('1 %', [(4, 0, 900000.0, 0.0)], cfg(carrier_hz=1.0e7)),
           ('half_taps', ok, cfg(half_taps=-1)), ('half_taps', ok, cfg(half_taps=33)), ('coh_ms', ok, cfg(coh_ms=-1)),
           ('coh_ms', ok, cfg(coh_ms=21)), ('n_runs', ok, cfg(n_runs=-1)), ('reserved', ok, cfg(reserved=1)),
           ('carrier_hz', ok, cfg(carrier_hz=nan)), ('carrier_hz', ok, cfg(carrier_hz=-1.0)),
           ('f_offset_hz', ok, cfg(f_offset_hz=inf)), ('no run', [(4, 19, 0.0, 0.0)], cfg(coh_ms=20, half_taps=8))]
    reason = {'nsat': 'nsat out of range 1..64', 'prn': 'prn out of range 1..37', 'skip_ms': 'skip_ms out of range 0..19',
              'f_hz': 'f_hz out of range', 'tau': 'tau out of range', '1 %': 'f_hz - f_offset_hz beyond 1 % of carrier_hz',
              'half_taps': 'half_taps out of range 1..32 (0: the default)', 'coh_ms': 'coh_ms out of range 1..20 (0: 20)',
              'n_runs': 'n_runs must be >= 1 (0: every run that fits)', 'reserved': 'a reserved field is not 0',
              'carrier_hz': 'carrier_hz must be positive (0: L1)', 'f_offset_hz': 'f_offset_hz must be finite',
              'no run': 'a record has no run inside iq'}
    for word, sats, c in bad:
        n_here = 38 * 2048 if word == 'no run' else n          # 37 windows fit, 19 are skipped: 18 < 20
        rc, msg = _plan_rc(2048, n_here, sats, c)
        assert rc == -1 and msg == 'gpsmi_acq_profile: ' + reason[word], (word, rc, msg)
    for n_bad in (0, (1 << 40) + 1):
        assert _plan_rc(2048, n_bad, ok, None) == (-1, 'gpsmi_acq_profile: n out of range 1..2^40')
    lib = _lib.load()
    assert lib.gpsmi_acq_profile_plan(2048, n, None, 1, None, None, None, None) == -1
    assert lib.gpsmi_last_error().decode() == 'gpsmi_acq_profile: null argument'
    for cs in (4096, 1024, 16384):
        assert _plan_rc(cs, n, ok, None) == (-5, f'gpsmi_acq_profile: code_samples 2048 and 16368 only ({cs})')
    with pytest.raises(engine.EngineError):
        engine.profiles_plan(2048, n, ok, half_taps=40)


@pytest.mark.parametrize('cs,which,Lh,coh', [(2048, 'short', 1, 1), (2048, 'short', 8, 3), (2048, 'short', 32, 1),
                                             (2048, 'long', 8, 20), (2048, 'long', 32, 3), (16368, 'short', 32, 3),
                                             (16368, 'short', 5, 1), (2048, 'long', 0, 0), (16368, 'short', 0, 2)])
def test_plan_counts_the_runs(cs, which, Lh, coh):
    n = R.KERNEL_N[cs, which]
    half = Lh or R.default_half(cs)
    sats = R.kernel_records(cs, n, half)
    runs, max_runs, K = engine.profiles_plan(cs, n, sats, Lh, coh)
    want = [len(R.prof_windows(n, cs, f, tau, half, skip, coh or 20)) for _, skip, f, tau in sats]
    assert runs.tolist() == want and max_runs == max(want) and K == 2 * half + 1
    limited, max_l, _ = engine.profiles_plan(cs, n, sats, Lh, coh, n_runs=1)
    assert limited.tolist() == [1] * len(sats) and max_l == 1
    # the flush record's last window ends with the input: one sample less and it is gone
    prn, skip, f, tau = sats[4]
    w = R.prof_windows(n, cs, f, tau, half, 0, 1)
    assert w[-1, 0] + cs + half == n
    assert len(R.prof_windows(n - 1, cs, f, tau, half, 0, 1)) == len(w) - 1
    assert engine.profiles_plan(cs, n - 1, [(prn, 0, f, tau)], Lh, 1)[0][0] == len(w) - 1


def test_skip_follows_the_bit_edge():
    """profile_sats: the first kept window starts a bit, whatever half_taps takes away in front."""
    cs = 2048
    m = np.zeros(3, S.MEAS_DTYPE)
    m['prn'], m['f_hz'], m['sample'] = [4, 5, 9], [1000.0, -2000.0, 0.0], 0
    m['code_phase'] = [3.25, 1500.5, 700.0]
    Tc = cs / (1.0 + m['f_hz'] / 1575.42e6)
    m['edge'] = m['code_phase'] + np.array([7, 0, 19]) * Tc
    m['edge'][2] = np.nan
    for Lh in (1, 8, 32):
        sats = profile_sats(m, cs, Lh)
        # record 0: tau 3.25 loses window 0 from Lh = 8 on
        assert [s[1] for s in sats] == [7 if Lh == 1 else 6, 0, 0]
        for (prn, skip, f, tau), r in zip(sats[:2], m[:2]):
            w = R.prof_windows(45 * cs, cs, f, tau, Lh, skip, 20)
            k = (w[0, 0] - r['edge']) / (cs / (1.0 + f / 1575.42e6))
            assert abs(k - np.rint(k)) < 1e-3 and int(np.rint(k)) % 20 == 0


# ---------------------------------------------------------------- the restatement's properties
def _one_path(noise, frac=0.0, f=1250.0, seconds=1.0, amp=0.0434, data_bits=True):
    """One satellite without code Doppler (delay_rate 0, Tc = cs by f_offset = f_hz), float samples."""
    cs = 2048
    sc = synth.Scene(sats=[synth.Sat(prn=4, doppler=f, delay=300.0 + frac, amp=amp, delay_rate=0.0,
                                     data_bits=data_bits)], seed=5,
                     noise_sigma=noise, code_samples=cs)
    x = sc.block_float(0, n=int(seconds * 1000) * cs)
    return R.prof_ref(x, [(4, 0, f, 300.0 + frac)], cs, f_offset=f)


def _whiten(Q, prn, cs, Lh):
    Lc = np.linalg.cholesky(S.profile_noise(prn, cs, Lh))
    return np.linalg.solve(Lc, np.linalg.solve(Lc, Q).conj().T).conj().T


def test_one_clean_path_is_rank_one_plus_noise():
    Sm, Q, n_runs = _one_path(0.35)
    assert n_runs.tolist() == [49]
    lam = np.sort(np.linalg.eigvalsh(_whiten(Q[0], 4, 2048, 8)))[::-1]
    print('whitened eigenvalues over their median:', np.round(lam / np.median(lam), 2))
    # 17 dimensions, 49 runs: white noise spreads its eigenvalues over (1 -+ sqrt(17 / 49))^2 of the mean
    assert lam[0] > 50.0 * lam[1] and lam[1] < 4.0 * np.median(lam) and lam[-1] > 0
    fit = S.profile_fit(Q[0], n_runs[0], 4, 0.0, 2048, 8, smear=0.0)
    print(fit)
    assert 0.5 < fit.T < 2.5 and fit.snr1 > 100 and fit.d1 == 0.0


def test_noiseless_single_path_has_no_second():
    """E2x at rounding level: against the exact templates of whole-sample delays (the replica's own
    circular autocorrelation) what is left is the complex64 rounding of the sums and the 24-bit
    carrier; against the analytic template, the float32 grid the replica is sampled on.  (Without
    data bits: a bit that changes next to a run turns the few samples the outer taps reach into the
    neighbouring period, 1e-8 of the energy, which is no rounding.)"""
    cs, Lh = 2048, 8
    Sm, Q, n_runs = _one_path(0.0, data_bits=False)
    Rr = R.replica64(4, cs)
    r = np.array([Rr @ np.roll(Rr, -k) for k in range(-Lh - 2, Lh + 3)])          # r[k + Lh + 2] = sum R[i] R[i + k]
    d = np.arange(-2.0, 3.0)
    g = np.stack([[r[(l - int(dd)) + Lh + 2] for l in range(-Lh, Lh + 1)] for dd in d])
    exact = S.profile_fit(Q[0], n_runs[0], 4, 0.0, cs, Lh, template=(d, g), smear=0.0)
    print('exact templates: E2x / E1 = %.3e' % (exact.e2x / exact.e1))
    assert exact.d1 == 0.0 and exact.e2x <= 1e-12 * exact.e1
    analytic = S.profile_fit(Q[0], n_runs[0], 4, 0.0, cs, Lh, smear=0.0)
    print('analytic template: E2x / E1 = %.3e' % (analytic.e2x / analytic.e1))
    assert analytic.d1 == 0.0 and analytic.e2x <= 1e-6 * analytic.e1


def test_plain_float32_is_close_and_not_equal():
    """The yardstick of the GPU tolerance: a float32 evaluation deviates, by 1e-5 at the most."""
    for cs, which, Lh, coh in ((2048, 'short', 8, 3), (16368, 'short', 5, 1)):
        ref = R.kernel_reference(cs, which, Lh, coh)
        p32 = R.kernel_reference(cs, which, Lh, coh, plain32=True)
        d_s, d_q = R.deviation(p32[0], p32[1], ref[0], ref[1])
        assert 0 < d_s < 1e-5 and 0 < d_q < 1e-5 and np.array_equal(ref[2], p32[2])


# ---------------------------------------------------------------- profile_fit on constructed covariances
CS, LH, RUNS, SIGMA2 = 2048, 8, 49, 3.0


def _built(paths, template=None):
    """Q = sum over the histories of a a^H + RUNS SIGMA2 N: `paths` is a list of histories, each a
    list of (power, delay) that share one phase history."""
    d, g = S.profile_template(4, CS, LH) if template is None else template
    Q = RUNS * SIGMA2 * S.profile_noise(4, CS, LH).astype(np.complex128)
    for hist in paths:
        a = sum(np.sqrt(p) * np.exp(0.7j * k) * g[int(np.argmin(np.abs(d - dd)))] for k, (p, dd) in enumerate(hist))
        Q = Q + RUNS * np.outer(a, a.conj())
    return Q


def test_fit_one_path():
    for smear in (0.0, None):
        f = S.profile_fit(_built([[(4.0e-4, 0.25)]]), RUNS, 4, 0.25, CS, LH, smear=smear)
        # (three directions hold all but 1e-5 of a template within half a sample: at an snr1 of 460
        # the rest reads as 0.005 of a noise dimension)
        tol = 1e-6 if smear == 0.0 else 1e-2
        assert f.T == pytest.approx(1.0, abs=tol) and f.sigma2 == pytest.approx(SIGMA2, rel=tol)
        assert f.d1 == 0.25 and f.snr1 > 100 and f.prn == 4 and f.n_runs == RUNS and f.frac == 0.25
    with pytest.raises(ValueError):
        S.profile_fit(np.eye(5), RUNS, 4, 0.0, CS, LH)


@pytest.mark.parametrize('same_history', [True, False])
def test_fit_two_paths(same_history):
    one = [(4.0e-4, 0.0)]
    two = [(4.0e-4, 0.0), (8.0e-4, 2.0)]
    t_one = S.profile_fit(_built([one]), RUNS, 4, 0.0, CS, LH).T
    f = S.profile_fit(_built([two] if same_history else [[p] for p in two]), RUNS, 4, 0.0, CS, LH)
    print(same_history, f)
    assert t_one == pytest.approx(1.0, abs=1e-2) and f.T > 50.0
    # the stronger path first; one template fitted to a coherent sum is drawn towards the other path
    assert abs(f.d1 - 2.0) <= 0.5 and abs(f.d2 - 0.0) <= 0.5
    assert 0.3 < f.rel_power < 0.7                                          # 4 : 8 in power
    # the rank-one model sees the same second path
    assert S.profile_fit(_built([two]), RUNS, 4, 0.0, CS, LH, smear=0.0).T > 50.0
    # within the sweep of whole-sample windows a second delay is the first one's: no flag
    near = [(4.0e-4, 0.0), (4.0e-4, 0.25)]
    assert S.profile_fit(_built([[p] for p in near]), RUNS, 4, 0.0, CS, LH).T < 2.0


def test_fit_with_an_override_template():
    """A front end that rounds the peak: the analytic template leaves a remainder that reads as a
    second path; the front end's own template explains the profile."""
    d, g = S.profile_template(4, CS, LH)
    k = np.array([0.25, 0.5, 0.25])
    rounded = np.stack([np.convolve(np.pad(row, 1, mode='edge'), k, mode='valid') for row in g])
    Q = _built([[(4.0e-4, 0.0)]], template=(d, rounded))
    assert S.profile_fit(Q, RUNS, 4, 0.0, CS, LH, smear=0.0).T > 3.0
    f = S.profile_fit(Q, RUNS, 4, 0.0, CS, LH, template=(d, rounded), smear=0.0)
    assert f.T == pytest.approx(1.0, abs=1e-6) and f.d1 == 0.0
    with pytest.raises(ValueError):
        S.profile_fit(Q, RUNS, 4, 0.0, CS, LH, template=(d, rounded[:, :5]))


def test_template_and_noise():
    d, g = S.profile_template(4, CS, LH)
    assert len(d) == 97 and d[0] == -3.0 and d[-1] == 3.0 and d[48] == 0.0 and g.shape == (97, 17)
    N = S.profile_noise(4, CS, LH)
    # g_0 is the replica's circular autocorrelation, to the float32 grid it is sampled on; the noise
    # colour is the linear one (a window holds no second period)
    Rr = R.replica64(4, CS)
    circ = np.array([Rr @ np.roll(Rr, -k) for k in range(-LH, LH + 1)])
    lin = np.array([Rr[abs(k):] @ Rr[:CS - abs(k)] for k in range(-LH, LH + 1)])
    assert np.abs(g[48] - circ).max() < 2e-4 * CS and np.abs(N[LH] * CS - lin).max() < 1e-9 and N[0, 0] == pytest.approx(R.replica64(4, CS) @ R.replica64(4, CS) / CS)
    assert np.all(np.linalg.eigvalsh(N) > 0)
    d16, g16 = S.profile_template(4, 16368, 2)
    assert d16[-1] == pytest.approx(3.0 * 16368 / 2048) and g16.shape == (97, 5)


# ---------------------------------------------------------------- the restated chain on the three scenes
def _profiled(which):
    """-> (records, report with the profile verdict, the records' bytes before the profiles)."""
    from test_snapshot_spoof import restated
    if which == 'liftoff':
        out, rep = LT.restated()
        x = synth.raw_to_c64(LT.raw())
    else:
        out, rep, _ = restated(which == 'spoofed')
        x = synth.raw_to_c64(ST.raw()) if which == 'spoofed' else T.c64('strong')
    before, rep = out.tobytes(), copy.copy(rep)
    cs = 2048
    _, Q, n_runs = R.prof_ref(x, profile_sats(out, cs), cs)
    S.profile_verdict(rep, out, Q, n_runs, cs, R.default_half(cs))
    print(which, 'doubled', rep.doubled, 'distorted', rep.distorted, 'alarm', rep.alarm)
    for m, f in zip(out, rep.profile):
        print('  PRN %2d  %.1f dB-Hz  T %8.2f  snr1 %7.0f  delays %+.2f %+.2f  second path %.2f'
              % (m['prn'], m['cn0_dbhz'], f.T, f.snr1, f.d1, f.d2, f.rel_power))
    return out, rep, before


def test_restated_scenes():
    """Where PROFILE_T_MIN comes from: twice the largest T over all records of the clean second and of
    the 30-us spoofed second (its copies lie 52 .. 67 lags away: the +- 8 taps must not see them);
    the lift-off second then shows SPOOF_MIN_DOUBLED or more PRNs at twice the threshold."""
    out_c, rep_c, before_c = _profiled('clean')
    out_s, rep_s, _ = _profiled('spoofed')
    out_l, rep_l, _ = _profiled('liftoff')
    t_max = max(rep_c.profile_t.max(), rep_s.profile_t.max())
    print('largest T without a copy inside the taps: %.3f (clean %.3f, 30 us %.3f); PROFILE_T_MIN %.2f'
          % (t_max, rep_c.profile_t.max(), rep_s.profile_t.max(), S.PROFILE_T_MIN))
    assert 2.0 * t_max <= S.PROFILE_T_MIN <= 2.0 * t_max * 1.005
    # the clean second: nothing flagged, and the records are the bytes they were (those of the chain
    # without the option: test_snapshot_spoof.py holds them to today's)
    assert rep_c.distorted == [] and rep_c.doubled == [] and not rep_c.alarm and len(rep_c.profile_t) == 8
    assert out_c.tobytes() == before_c
    from test_snapshot_spoof import restated
    _, info = T.strong()
    fixes = [S.twin_fixes(out_c, info['ephs'], info['t0_gps'] + ST.TIME_OFF, ST.apriori(), rep)
             for rep in (copy.copy(restated(False)[1]), rep_c)]
    assert fixes[0].ok and fixes[1].ok and fixes[1].ecef.tobytes() == fixes[0].ecef.tobytes()
    assert fixes[1].residuals.tobytes() == fixes[0].residuals.tobytes() and fixes[1].t_gps == fixes[0].t_gps
    assert fixes[1].prns == fixes[0].prns and rep_c.fixes[1] is None
    # the 30-us second: every PRN doubled, none distorted
    assert rep_s.distorted == [] and len(rep_s.doubled) == 8 and rep_s.alarm and len(rep_s.profile_t) == 16
    # the lift-off second: one record per PRN (every copy inside the guard), the alarm from the profiles
    off = LT.copy_offsets()
    print('copies behind the authentic codes, samples:', {p: round(v, 2) for p, v in off.items()})
    assert max(abs(v) for v in off.values()) < 2.05 and min(abs(v) for v in off.values()) > 0.1
    assert rep_l.doubled == [] and out_l['prn'].tolist() == sorted(off)
    assert rep_l.distorted == LT.REF_DISTORTED and rep_l.alarm
    clear = [int(m['prn']) for m, t in zip(out_l, rep_l.profile_t) if t >= 2.0 * S.PROFILE_T_MIN]
    assert len(clear) >= S.SPOOF_MIN_DOUBLED and set(clear) <= set(rep_l.distorted)
    assert all(f.snr1 >= S.PROFILE_SNR1_MIN for f in rep_l.profile)
    # without the profiles this second raises no alarm at all
    assert not LT.restated()[1].alarm


def test_a_standing_alarm_stays():
    """The profiles add to the alarm and never take it back: every signal from one direction and no
    doubled PRN (DESIGN.md 4.2p's one_direction) with clean profiles is still an alarm."""
    m = np.zeros(2, S.MEAS_DTYPE)
    m['prn'], m['code_phase'] = [4, 9], [10.25, 33.5]
    one = _built([[(4.0e-4, 0.0)]])
    rep = S.SpoofReport(doubled=[], one_direction=True, alarm=True)
    S.profile_verdict(rep, m, np.stack([one, one]), [RUNS] * 2, CS, LH)
    assert rep.distorted == [] and rep.profile_t.max() < S.PROFILE_T_MIN and rep.alarm and rep.one_direction
    rep = S.SpoofReport(doubled=[4, 9], alarm=True)                         # min_doubled 3 would not raise it anew
    assert S.profile_verdict(rep, m, np.stack([one, one]), [RUNS] * 2, CS, LH, min_doubled=3).alarm
    assert not S.profile_verdict(S.SpoofReport(), m, np.stack([one, one]), [RUNS] * 2, CS, LH).alarm


def test_profile_sats_takes_the_call_carrier():
    """The skip is counted on the windows the engine cuts: with another carrier_hz the code period is
    another one, and the first kept window still starts a bit."""
    from gpsmi.acquisition import Acquisition
    cs, carrier = 2048, 1.0e8
    m = np.zeros(1, S.MEAS_DTYPE)
    m['prn'], m['f_hz'], m['code_phase'] = 4, 4000.0, 1500.5
    Tc = cs / (1.0 + 4000.0 / carrier)
    m['edge'] = 1500.5 + 13 * Tc
    (prn, skip, f, tau), = profile_sats(m, cs, 8, carrier_hz=carrier)
    w = R.prof_windows(45 * cs, cs, f, tau, 8, skip, 20, carrier_hz=carrier)
    k = (w[0, 0] - m['edge'][0]) / Tc
    assert skip == 13 and abs(k - np.rint(k)) < 1e-3 and int(np.rint(k)) % 20 == 0
    seen = {}

    class Eng:
        def profiles(self, data, sats, **kw):
            seen.update(sats=sats, kw=kw)
            return 'cov', 'runs'
    a = Acquisition.__new__(Acquisition)
    a.engine, a.cfg = Eng(), type('Cfg', (), {'code_samples': cs})()
    assert a.profileHits(None, m, half_taps=8, carrier_hz=carrier) == ('cov', 'runs')
    assert seen['sats'] == [(prn, skip, f, tau)] and seen['kw']['carrier_hz'] == carrier


def test_kernel_registers():
    """What the build reports for the tap-sum kernels (the compiler's resource remarks, as
    test_cu_budget.py reads them): no scratch and no accumulation registers in any form; the 65-tap
    form stays at two waves per SIMD -- its loop holds the LDS reads eight ahead of their use by a
    scheduling hint, and without it the sums spill (256 VGPRs and 72 AGPRs, one wave)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import cu_budget as cb
    path = os.path.join(cb.BUILD, 'gpsmi_acq.resources')
    if not os.path.exists(path) or cb.cxxfilt() is None:
        pytest.skip('no resource remarks from a build, or no c++filt to read the kernel names with')
    k = cb.parse([path])
    for fmt in (0, 1):
        small, big = k[f'prof_sum_kernel<{fmt}, 8>'], k[f'prof_sum_kernel<{fmt}, 32>']
        print(fmt, small, big)
        assert small['scratch'] == big['scratch'] == 0 and small['agpr'] == big['agpr'] == 0
        assert small['vgpr'] <= 128 and small['waves'] >= 4 and small['lds'] <= 40 * 1024
        assert big['vgpr'] <= 256 and big['waves'] >= 2 and big['lds'] <= 48 * 1024
    assert k['prof_cov_kernel']['scratch'] == 0 and k['prof_cov_kernel']['lds'] == 0


def test_verdict_rules():
    rep = S.SpoofReport(doubled=[7])
    m = np.zeros(3, S.MEAS_DTYPE)
    m['prn'], m['code_phase'] = [4, 4, 9], [10.25, 500.0, 33.5]
    weak = _built([[(1.0e-5, 0.0), (1.0e-5, 2.0)]])                                  # two paths below the floor
    two = _built([[(4.0e-4, 0.0)], [(4.0e-4, 2.0)]])
    one = _built([[(4.0e-4, 0.0)]])
    S.profile_verdict(rep, m, np.stack([one, two, weak]), [RUNS] * 3, CS, LH)
    assert rep.profile_t[0] < S.PROFILE_T_MIN < rep.profile_t[1] and rep.profile[2].snr1 < S.PROFILE_SNR1_MIN
    assert rep.distorted == [4] and rep.alarm and rep.profile[0].frac == 0.25          # 7 doubled, 4 distorted
    assert not S.profile_verdict(S.SpoofReport(), m, np.stack([one, two, weak]), [RUNS] * 3, CS, LH).alarm
    with pytest.raises(ValueError):
        S.snapshot_fix(None, np.zeros(8), {}, 0.0, profile=True)                     # (with spoof only)
