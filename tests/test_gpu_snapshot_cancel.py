"""gpsmi.snapshot.measure(cancel=...) on the GPU: the collision scene of
cancel_ref.py -- three satellites at 53 dB-Hz and PRN 3 at amplitude 0.00772 (30 dB-Hz) 2 Hz from
PRN 4 modulo 1 kHz, 16 blocks = 0.512 s -- where the weak satellite is measured only once the
strong ones are cancelled (tests/test_snapshot_cancel.py checks the same outcome on the float64
restatements), and the scenes of snapshot_truth.py, where `cancel=None` must stay what it was and
`cancel=True` must keep every satellite and not raise the fix error."""
import numpy as np
import pytest

import cancel_ref as R
import snapshot_truth as T
from gpsmi import snapshot as S
from test_gpu_snapshot import TIME_OFF, acqs, bound, report  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def collision():
    from gpsmi.synth import raw_to_c64
    raw = R.collision_raw()
    return raw_to_c64(raw), raw


@pytest.mark.parametrize('raw', [False, True], ids=['c64', 'u8'])
def test_collision_scene(acqs, collision, raw):
    acq, data = acqs[int(raw)], collision[int(raw)]
    st0, st1 = {}, {}
    before = S.measure(acq, data, prns=R.COLLISION_PRNS, source='refine', stats=st0)
    after = S.measure(acq, data, prns=R.COLLISION_PRNS, source='refine', stats=st1, cancel=True)
    for name, meas, st in (('without', before, st0), ('cancel=True', after, st1)):
        print(name, [(int(m['prn']), round(float(m['code_phase']), 3), round(float(m['f_hz']), 2),
                      round(float(m['cn0_dbhz']), 1)) for m in meas], '%.3f ms' % st['device_ms'])
        print('  found', [(round(h[0], 2), h[1], h[2], h[3]) for h in st['found']])
    assert acq.engine.raw_u8 == raw                       # the input format is what it was
    assert 3 not in before['prn'].tolist() and 'cancelled' not in st0
    assert after['prn'].tolist() == [3, 4, 5, 9]
    p, f, d = R.COLLISION_WEAK
    weak = after[0]
    print('PRN 3: code phase %.3f (truth %.3f), Doppler %.2f (truth %.1f)' % (weak['code_phase'], R.true_tau(f, d),
                                                                              weak['f_hz'], f))
    assert abs(weak['code_phase'] - R.true_tau(f, d)) <= 0.25 and abs(weak['f_hz'] - f) <= 5.0
    c = st1['cancelled']
    ratio = c['energy_removed'] / c['energy_in']
    print('cancelled', c['prn'].tolist(), 'removed / in', np.round(ratio, 4), 'skipped', c['n_skipped'].tolist())
    assert sorted(c['prn'].tolist()) == [4, 5, 9]
    assert np.all((ratio > 0.02) & (ratio < 0.2))
    assert st1['device_ms'] > 0 and st0['device_ms'] > 0
    # the kept satellites' records are the first pass's
    for prn in (4, 5, 9):
        assert before[before['prn'] == prn].tobytes() == after[after['prn'] == prn].tobytes()
    # a threshold nothing reaches: the first pass alone
    none = S.measure(acq, data, prns=R.COLLISION_PRNS, source='refine', cancel=70.0, stats=st0)
    assert none.tobytes() == before.tobytes() and len(st0['cancelled']) == 0


def todays_measure(acq, data, prns, f_offset=0.0):
    """measure() as it was before `cancel` existed, stage by stage: source 'track', default options."""
    from gpsmi.engine import DeviceBuffer
    from gpsmi.pipeline import largest_peak_hits, refine_centred
    c = acq.cfg
    cs, n = c.code_samples, len(data)
    freqs = [c.min_freq + c.step_freq * i for i in range(int(round((c.max_freq - c.min_freq) / c.step_freq)))]
    n_seg = n // cs // 4
    host = acq.engine._host_iq(data)
    buf = DeviceBuffer(host.nbytes, c.device)
    try:
        buf.upload(host)
        dev = (buf.ptr, n)
        found = largest_peak_hits(acq, (dev[0], n_seg * 4 * cs), prns, freqs, 4, n_seg, f_offset=f_offset,
                                  corr_min=c.corr_min)
        found, rec, _ = refine_centred(acq, dev, found, f_offset=f_offset)
        rec, found, out = S.refined_records(rec, found, cs, f_offset)
        bits, states = acq.trackHits(dev, rec, f_offset=f_offset)
        S.tracked_records(out, bits, states['bit_no'], n, cs, 0)
        return out[np.argsort(out['prn'], kind='stable')]
    finally:
        buf.free()


@pytest.mark.parametrize('name', ['strong', 'mixed'])
def test_existing_scenes_without_cancel_are_unchanged(acqs, name):
    _, info = getattr(T, name)()
    prns = sorted(info['ephs'])
    raw = np.ascontiguousarray(T.raw(name))
    want = todays_measure(acqs[1], raw, prns)
    assert len(want) == len(prns)
    stats = {}
    for cancel in (None, False):
        assert S.measure(acqs[1], raw, prns=prns, cancel=cancel, stats=stats).tobytes() == want.tobytes()
        assert 'cancelled' not in stats
    assert S.measure(acqs[1], raw, prns=prns).tobytes() == want.tobytes()


def test_mixed_scene_with_cancel_keeps_the_weak_satellites(acqs):
    """MI355X: the fix is 417.28 m from the truth with cancel=True (419.55 m without, 419.6 m in
    T.REF); the weak three's code-phase errors are -0.079 / 0.043 / -0.018 sample with and -0.070 /
    0.036 / 0.001 without -- at 35 dB-Hz these satellites are not limited by the strong ones, and
    what cancelling changes for them is within their noise, in either direction."""
    sc, info = T.mixed()
    data = T.c64('mixed')
    prns = sorted(info['ephs'])
    plain = S.measure(acqs[0], data, prns=prns)
    stats = {}
    fix, meas, ms = S.snapshot_fix(acqs[0], data, info['ephs'], info['t0_gps'] + TIME_OFF, cancel=True, stats=stats)
    err, pe, fe = report('mixed, cancel=True', sc, fix, meas, ms, len(data))
    pe0 = T.phase_error(sc, plain)
    weak = np.isin(meas['prn'], T.MIXED_WEAK)
    print('code phase errors of the weak three: %s with cancel, %s without; cancelled %s'
          % (np.round(pe[weak], 3), np.round(pe0[weak], 3), stats['cancelled']['prn'].tolist()))
    assert meas['prn'].tolist() == prns == plain['prn'].tolist() and len(meas) == 6
    assert sorted(stats['cancelled']['prn'].tolist()) == sorted(set(prns) - set(T.MIXED_WEAK))
    assert {s.decode() for s in meas['source']} == {'track'}
    # the uncancelled figure T.REF records for this scene is the fix error of the chain, which the
    # weak three's code phases govern (g = 23): cancelling must not raise it; the code phases
    # themselves are held to the quarter sample every measurement of these scenes is held to
    assert fix.ok and len(fix.prns) == 6 and bound('mixed', None, 'track', fix.g) > 0
    assert err <= T.REF['mixed', None, 'track'][0]
    assert np.abs(pe[weak]).max() <= 0.25
