"""GPU: snapshot_fix(..., spoof=True) on the two scenes of test_snapshot_spoof.py.

The spoofed scene: all eight PRNs doubled, two fixes that are ok, each within min(2 x the
restatement's error, g x a quarter of a sample) of its own position -- test_gpu_snapshot.py's rule,
with spoof_truth.REF measured on the CPU.  The clean scene: no alarm, and the Fix and the
measurements of the option are the bytes of a call without it.

The first test that asks for it synthesises the spoofed second on the host (sixteen signals,
spoof_truth.raw, shared with test_run_file_spoof.py): about ten seconds that are not device time."""
import numpy as np
import pytest

import snapshot_truth as T
import spoof_truth as ST
from gpsmi import snapshot as S
from test_gpu_snapshot import QUARTER_SAMPLE_M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def acq():
    from gpsmi.acquisition import Acquisition
    a = Acquisition(raw_u8=True)
    yield a
    a.engine.close()


def bound(which, g):
    ref_err, ref_g = ST.REF[which]
    assert abs(g - ref_g) <= 0.01 * ref_g
    return min(2.0 * ref_err, g * QUARTER_SAMPLE_M)


def test_spoofed_scene(acq):
    _, info, _ = ST.spoofed()
    stats = {}
    fix, meas, ms = S.snapshot_fix(acq, ST.raw(), info['ephs'], info['t0_gps'] + ST.TIME_OFF, pos=ST.apriori(),
                                   source='refine', spoof=True, stats=stats)
    rep = fix.spoof
    assert rep is stats['spoof'] and rep.fixes[0] is fix
    z = np.sort(rep.picks['z'], axis=1)[:, ::-1]
    print('z of the two copies %.1f .. %.1f, of the best further pick %.1f; %d hits refined; %.3f ms peaks of %.2f ms' % (
        z[:, :2].min(), z[:, :2].max(), z[:, 2:].max(), len(stats['found']), stats['peaks_ms'], ms))
    assert rep.doubled == sorted(info['ephs']) and len(rep.doubled) == 8 and rep.alarm
    assert meas['prn'].tolist() == sorted(2 * sorted(info['ephs']))
    fa, fb = rep.fixes
    assert fa.ok and fb.ok, (fa.reason, fb.reason)
    err = {'truth': np.linalg.norm(fa.ecef - T.TRUTH), 'spoofer': np.linalg.norm(fb.ecef - ST.spoofer_pos())}
    print('fix_a %.2f m from the truth (g %.3f, %d satellites), fix_b %.2f m from the spoofer (g %.3f, %d satellites), '
          'separation %.1f m' % (err['truth'], fa.g, len(fa.prns), err['spoofer'], fb.g, len(fb.prns), rep.separation_m))
    assert err['truth'] <= bound('truth', fa.g)
    assert err['spoofer'] <= bound('spoofer', fb.g)


@pytest.mark.parametrize('source', ['refine', 'track'])
def test_clean_scene_is_the_same_bytes(acq, source):
    _, info = T.strong()
    raw = T.raw('strong')
    args = (acq, raw, info['ephs'], info['t0_gps'] + ST.TIME_OFF)
    fix0, meas0, _ = S.snapshot_fix(*args, pos=ST.apriori(), source=source)
    fix, meas, _ = S.snapshot_fix(*args, pos=ST.apriori(), source=source, spoof=True)
    rep = fix.spoof
    assert rep.doubled == [] and not rep.alarm and not rep.crowded and rep.fixes[0] is fix and rep.fixes[1] is None
    assert meas.tobytes() == meas0.tobytes() and len(meas) == 8
    assert fix.ok and fix0.ok and fix0.spoof is None
    for k in ('ecef', 'residuals', 'integers', 'tau', 'slope'):
        assert getattr(fix, k).tobytes() == getattr(fix0, k).tobytes()
    for k in ('t_gps', 'sample', 'bias_m', 'prns', 'ref_prn', 'dropped', 'g', 'rms_m', 'test_m', 'protect_m', 'moved_m',
              'iterations', 'path'):
        assert getattr(fix, k) == getattr(fix0, k)


def test_option_off_is_unchanged(acq):
    """measure without the option returns records alone, as before; with it, the pair."""
    _, info = T.strong()
    prns = sorted(info['ephs'])
    raw = T.raw('strong')[:T.TWO_BLOCKS]
    ref = S.measure(acq, raw, prns=prns)
    assert isinstance(ref, np.ndarray) and ref.dtype == S.MEAS_DTYPE and len(ref) == 8
    assert S.measure(acq, raw, prns=prns, spoof=False).tobytes() == ref.tobytes()
    meas, rep = S.measure(acq, raw, prns=prns, spoof=True)
    assert meas.tobytes() == ref.tobytes() and rep.doubled == [] and rep.picks.shape == (8, S.SPOOF_PICKS)
    with pytest.raises(ValueError):
        S.measure(acq, raw, prns=prns, spoof=True, cancel=True)
