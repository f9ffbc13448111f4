"""GPU: snapshot_fix(..., spoof=True, profile=True) on the lift-off second
(liftoff_truth.py) and on the clean second.

The lift-off second: no PRN is doubled -- every copy lies inside the guard of the peaks -- and the
profiles raise the alarm with the verdict of the restated chain (liftoff_truth.REF_DISTORTED, measured
and asserted on the CPU by test_profile.py).  T of every record is held to the restatement
(profile_ref.py) of the profiles of the same records, within four times the relative distance at which
a plain numpy float32 evaluation of those profiles puts its T from the float64 one: the kernel
tolerance of test_gpu_profile.py carried through profile_fit.  The clean second: nothing flagged, and
the Fix, the measurements and the rest of the report are the bytes of a call without the option.
With four antennas (and beams) on 64 ms: everything else of the report is the bytes of a call without
the profiles, and an alarm that stands is not taken back.

The first test synthesises the lift-off second on the host (sixteen signals): about ten seconds that are
not device time."""
import numpy as np
import pytest

import liftoff_truth as LT
import profile_ref as R
import snapshot_truth as T
import spoof_truth as ST
from gpsmi import snapshot as S
from gpsmi.acquisition import profile_sats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def acq():
    from gpsmi.acquisition import Acquisition
    a = Acquisition(raw_u8=True)
    yield a
    a.engine.close()


def test_liftoff_second(acq):
    from gpsmi.synth import raw_to_c64
    _, info, _ = LT.liftoff()
    stats = {}
    fix, meas, ms = S.snapshot_fix(acq, LT.raw(), info['ephs'], info['t0_gps'] + ST.TIME_OFF, pos=ST.apriori(),
                                   source='refine', spoof=True, profile=True, stats=stats)
    rep = fix.spoof
    assert rep is stats['spoof'] and stats['profile_ms'] > 0 and ms >= stats['profile_ms']
    print('profiles of %d records: %.3f ms of %.2f ms on the device' % (len(meas), stats['profile_ms'], ms))
    assert rep.doubled == [] and meas['prn'].tolist() == sorted(info['ephs'])
    assert rep.distorted == LT.REF_DISTORTED and rep.alarm
    assert fix.ok and rep.fixes[0] is fix and rep.fixes[1] is None         # one fix, already being pulled
    # T against the restatement of the same records' profiles
    cs = 2048
    x = raw_to_c64(LT.raw())
    sats = profile_sats(meas, cs)
    _, Q, n_runs = R.prof_ref(x, sats, cs)
    _, Q32, _ = R.prof_ref(x, sats, cs, plain32=True)
    t_ref, t_32 = (np.array([S.profile_fit(q[r], n_runs[r], meas['prn'][r], 0.0, cs, 8).T for r in range(len(meas))])
                   for q in (Q, Q32))
    tol = 4.0 * np.abs(t_32 / t_ref - 1.0).max()
    dev = np.abs(rep.profile_t / t_ref - 1.0).max()
    for m, t, tr in zip(meas, rep.profile_t, t_ref):
        print('  PRN %2d  T %9.3f  restated %9.3f' % (m['prn'], t, tr))
    print('largest relative distance of T from its restatement %.3e, bound %.3e' % (dev, tol))
    assert np.array_equal(n_runs, [f.n_runs for f in rep.profile])
    assert 0 < tol < 1e-2 and dev <= tol
    clear = [int(m['prn']) for m, t in zip(meas, rep.profile_t) if t >= 2.0 * S.PROFILE_T_MIN]
    assert len(clear) >= S.SPOOF_MIN_DOUBLED


@pytest.mark.parametrize('source', ['refine', 'track'])
def test_clean_second_is_the_same_bytes(acq, source):
    _, info = T.strong()
    args = (acq, T.raw('strong'), info['ephs'], info['t0_gps'] + ST.TIME_OFF)
    st0, st = {}, {}
    fix0, meas0, _ = S.snapshot_fix(*args, pos=ST.apriori(), source=source, spoof=True, stats=st0)
    fix, meas, _ = S.snapshot_fix(*args, pos=ST.apriori(), source=source, spoof=True, profile=True, stats=st)
    rep0, rep = fix0.spoof, fix.spoof
    print(source, 'T', np.round(rep.profile_t, 2))
    assert rep.distorted == [] and rep.doubled == [] and not rep.alarm and len(rep.profile_t) == 8
    assert rep.profile_t.max() < S.PROFILE_T_MIN and all(f.snr1 >= S.PROFILE_SNR1_MIN for f in rep.profile)
    assert rep0.profile_t is None and rep0.profile is None and rep0.distorted == [] and 'profile_ms' not in st0
    assert meas.tobytes() == meas0.tobytes() and st['refined'].tobytes() == st0['refined'].tobytes()
    assert rep.picks.tobytes() == rep0.picks.tobytes() and rep.prns == rep0.prns and rep.crowded == rep0.crowded
    assert fix.ok and fix0.ok
    for k in ('ecef', 'residuals', 'integers', 'tau', 'slope'):
        assert getattr(fix, k).tobytes() == getattr(fix0, k).tobytes()
    for k in ('t_gps', 'sample', 'bias_m', 'prns', 'ref_prn', 'dropped', 'g', 'rms_m', 'test_m', 'protect_m', 'moved_m',
              'iterations', 'path'):
        assert getattr(fix, k) == getattr(fix0, k)


def test_option_rules(acq):
    _, info = T.strong()
    raw = T.raw('strong')[:T.TWO_BLOCKS]
    with pytest.raises(ValueError):
        S.measure(acq, raw, prns=sorted(info['ephs']), profile=True)        # with spoof only
    meas, rep = S.measure(acq, raw, prns=sorted(info['ephs']), spoof=True, profile=True)
    # 64 ms hold two runs of 20 ms behind the bit edge
    assert len(rep.profile_t) == len(meas) == 8 and all(f.n_runs in (2, 3) for f in rep.profile)


@pytest.mark.parametrize('which,beams', [('spoofed', False), ('clean', True)])
def test_with_antennas_and_beams(acq, which, beams):
    """The profiles beside the signatures (and the beams) of DESIGN.md 4.2p / 4.2q on 64 ms over four
    antennas: the records, the signatures and the verdicts are the bytes of a call without the
    profiles, the alarm of the doubled PRNs stands, and the profiles are those of antenna 0 taken with
    the same records."""
    import sig_ref
    info = (ST.spoofed() if which == 'spoofed' else T.strong())[1]
    rows = sig_ref.snapshot_raw(which, T.TWO_BLOCKS // 2048)
    kw = dict(prns=sorted(info['ephs']), spoof=True, antennas=sig_ref.SNAP_ANTENNAS, **({'beams': True} if beams else {}))
    meas0, rep0 = S.measure(acq, rows, **kw)
    meas, rep = S.measure(acq, rows, profile=True, **kw)
    assert meas.tobytes() == meas0.tobytes() and rep.doubled == rep0.doubled and rep.one_direction == rep0.one_direction
    assert rep.signature.tobytes() == rep0.signature.tobytes() and rep.rho.tobytes() == rep0.rho.tobytes()
    assert rep0.profile_t is None and len(rep.profile_t) == len(meas) and np.all(np.isfinite(rep.profile_t))
    assert rep.alarm or not rep0.alarm                                       # never taken back
    assert rep.alarm == (rep0.alarm or len(set(rep.doubled) | set(rep.distorted)) >= S.SPOOF_MIN_DOUBLED)
    if which == 'spoofed':
        assert len(rep.doubled) == 8 and rep.alarm
    cov, runs = acq.profileHits(np.ascontiguousarray(rows[0]), meas)
    t = [S.profile_fit(cov[r], runs[r], meas['prn'][r], 0.0, 2048, 8).T for r in range(len(meas))]
    assert np.array_equal(rep.profile_t, t) and [f.n_runs for f in rep.profile] == runs.tolist()
