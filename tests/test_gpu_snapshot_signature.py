"""GPU: snapshot_fix(..., spoof=True, antennas=4) on the scenes of
test_snapshot_signature.py: the four-antenna spoofed scene -- both copies of all eight PRNs, the
verdict names the spoofer's set, the authentic fix comes first within the bound that
test_gpu_snapshot_spoof.py forms from spoof_truth.REF -- and the clean scene, whose Fix and
measurements are the bytes of the single-antenna call on row 0.

The first test that asks for a scene synthesises its second on the host for four antennas
(sig_ref.snapshot_raw, cached): seconds that are not device time."""
import numpy as np
import pytest

import sig_ref as R
import snapshot_truth as T
import spoof_truth as ST
from gpsmi import snapshot as S
from test_gpu_snapshot_spoof import bound
from test_snapshot_signature import is_added

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def acq():
    from gpsmi.acquisition import Acquisition
    a = Acquisition(raw_u8=True)
    yield a
    a.engine.close()


def test_spoofed_scene_names_the_spoofer(acq):
    _, info, _ = ST.spoofed()
    rows = R.snapshot_raw('spoofed')
    assert np.array_equal(rows[0], ST.raw())
    stats = {}
    # the a-priori beside the spoofer: twin_fixes alone would put the spoofer's fix first
    fix, meas, ms = S.snapshot_fix(acq, rows, info['ephs'], info['t0_gps'] + ST.TIME_OFF, pos=ST.spoofer_pos() + 100.0,
                                   source='refine', spoof=True, antennas=R.SNAP_ANTENNAS, stats=stats)
    rep = fix.spoof
    assert rep is stats['spoof'] and rep.fixes[0] is fix and rep.antennas == R.SNAP_ANTENNAS
    assert rep.doubled == sorted(info['ephs']) and len(rep.doubled) == 8 and rep.alarm
    assert meas['prn'].tolist() == sorted(2 * sorted(info['ephs']))
    assert 'signature_ms' in stats and 0 < stats['signature_ms'] <= ms
    spoofer = [i for i, r in enumerate(meas) if is_added(r)]
    authentic = [i for i in range(len(meas)) if i not in spoofer]
    assert len(spoofer) == 8
    rho = rep.rho
    same = min(rho[i, j] for k, i in enumerate(spoofer) for j in spoofer[k + 1:])
    auth = min(rho[i, j] for k, i in enumerate(authentic) for j in authentic[k + 1:])
    print('same-source pairs: least rho %.4f; authentic pairs: least %.4f; quality %.1f .. %.1f; signatures %.3f ms of '
          '%.2f ms' % (same, auth, rep.quality.min(), rep.quality.max(), stats['signature_ms'], ms))
    assert same >= S.SPOOF_RHO_MIN and auth < S.SPOOF_RHO_MIN
    assert rep.authentic == 0 and rep.one_source == (False, True) and not rep.one_direction
    assert set(rep.sets[1]) <= set(spoofer) and set(rep.sets[0]) <= set(authentic)
    fa, fb = rep.fixes
    assert fa.ok and fb.ok, (fa.reason, fb.reason)
    err = {'truth': np.linalg.norm(fa.ecef - T.TRUTH), 'spoofer': np.linalg.norm(fb.ecef - ST.spoofer_pos())}
    print('fixes[0] %.2f m from the truth (g %.3f), fixes[1] %.2f m from the spoofer (g %.3f)'
          % (err['truth'], fa.g, err['spoofer'], fb.g))
    assert err['truth'] <= bound('truth', fa.g)
    assert err['spoofer'] <= bound('spoofer', fb.g)


def test_clean_scene_is_the_same_bytes(acq):
    _, info = T.strong()
    rows = R.snapshot_raw('clean', T.TWO_BLOCKS // 2048)             # (64 ms: what test_gpu_snapshot_spoof's last test takes)
    assert np.array_equal(rows[0], T.raw('strong')[:T.TWO_BLOCKS])
    args = (acq, info['ephs'], info['t0_gps'] + ST.TIME_OFF)
    fix0, meas0, _ = S.snapshot_fix(args[0], np.ascontiguousarray(rows[0]), *args[1:], pos=ST.apriori(), source='refine',
                                    spoof=True)
    stats = {}
    fix, meas, _ = S.snapshot_fix(args[0], rows, *args[1:], pos=ST.apriori(), source='refine', spoof=True,
                                  antennas=R.SNAP_ANTENNAS, stats=stats)
    rep = fix.spoof
    assert rep.doubled == [] and not rep.alarm and not rep.one_direction and rep.authentic is None
    assert rep.fixes[0] is fix and rep.fixes[1] is None and rep.signature.shape == (8, R.SNAP_ANTENNAS)
    assert meas.tobytes() == meas0.tobytes() and len(meas) == 8 and stats['signature_ms'] > 0
    assert fix.ok and fix0.ok
    for k in ('ecef', 'residuals', 'integers', 'tau', 'slope'):
        assert getattr(fix, k).tobytes() == getattr(fix0, k).tobytes()
    for k in ('t_gps', 'sample', 'bias_m', 'prns', 'ref_prn', 'dropped', 'g', 'rms_m', 'test_m', 'protect_m', 'moved_m',
              'iterations', 'path'):
        assert getattr(fix, k) == getattr(fix0, k)


def test_antennas_go_with_spoof(acq):
    _, info = T.strong()
    rows = R.snapshot_raw('clean', T.TWO_BLOCKS // 2048)
    with pytest.raises(ValueError):
        S.snapshot_fix(acq, rows, info['ephs'], info['t0_gps'], pos=ST.apriori(), antennas=4)
    with pytest.raises(ValueError):
        S.measure(acq, rows, prns=sorted(info['ephs']), antennas=4)
    with pytest.raises(ValueError):
        S.measure(acq, rows, prns=sorted(info['ephs']), spoof=True, antennas=4, cancel=True)
    with pytest.raises(ValueError):
        S.snapshot_fix(acq, rows, info['ephs'], info['t0_gps'], pos=ST.apriori(), spoof=True, antennas=4, collective=True)
    with pytest.raises(ValueError):
        S.measure(acq, rows[:3], prns=sorted(info['ephs']), spoof=True, antennas=4)      # three rows are not four
