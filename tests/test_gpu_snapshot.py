"""gpsmi.snapshot on the GPU: deep search -> refinement -> tracking -> coarse-time fix on the
scenes of snapshot_truth.py, against the scenes' truth and the fix errors of the float64
restatement chain (tests/test_snapshot.py::test_restatement_chain, no a-priori position, time 20 s
off):

    scene                      source   restatement   g       bound = min(2 x, g * 0.25 sample * c / fs)
    strong, 1.0 s              track       7.69 m     1.91     15.4 m
    mixed, 1.2 s               track     419.6 m     22.94    839.2 m
    strong, 131072 samples     refine     10.98 m     1.91     22.0 m

MI355X (profiles/snapshot/gpu_tests.txt): strong 7.69 m (code phases within 0.089 sample, Dopplers
within 0.49 Hz, bit edges within 0.089 sample, 6.29 ms on the device), mixed 419.55 m (0.120 sample,
0.43 Hz, 6.65 ms), two blocks 10.98 m (0.198 sample, 1.48 Hz, 0.19 ms), 86017 samples 8 of 8 measured
(0.161 sample): the restatement's figures to the centimetre."""
import pickle

import numpy as np
import pytest

import snapshot_truth as T
from gpsmi import snapshot as S

pytestmark = pytest.mark.gpu

FS = 2048000.0
QUARTER_SAMPLE_M = 0.25 * S.P.GPS_C / FS
TIME_OFF = 20.0


@pytest.fixture(scope='module')
def acqs():
    from gpsmi.acquisition import Acquisition
    a, r = Acquisition(), Acquisition(raw_u8=True)
    yield a, r
    a.engine.close()
    r.engine.close()


def bound(name, n, source, g):
    ref_err, ref_g = T.REF[name, n, source]
    assert abs(g - ref_g) <= 0.01 * ref_g
    return min(2.0 * ref_err, g * QUARTER_SAMPLE_M)


def report(name, sc, fix, meas, ms, n):
    pe, fe = T.phase_error(sc, meas), T.doppler_error(sc, meas, n // 2)
    err = np.linalg.norm(fix.ecef - T.TRUTH) if fix.ok else float('nan')
    print('%s: %d measured, fix %s %.2f m from the truth (g %.3f, rms %.1f m, dropped %s), code phase errors %s, '
          'Doppler errors %s, cn0 %s, %.2f ms on the device' % (
              name, len(meas), fix.ok or fix.reason, err, fix.g, fix.rms_m, fix.dropped, np.round(pe, 3), np.round(fe, 2),
              np.round(meas['cn0_dbhz'], 1), ms))
    return err, pe, fe


def test_strong_scene_without_a_position(acqs):
    sc, info = T.strong()
    raw = T.raw('strong')
    fix, meas, ms = S.snapshot_fix(acqs[1], raw, info['ephs'], info['t0_gps'] + TIME_OFF)
    err, pe, fe = report('strong', sc, fix, meas, ms, len(raw))
    assert meas['prn'].tolist() == [2, 5, 8, 10, 13, 16, 19, 21] and ms > 0
    assert np.abs(pe).max() <= 0.25 and np.abs(fe).max() <= 5.0
    assert {s.decode() for s in meas['source']} == {'track'}
    ee = T.edge_error(sc, meas)
    print('bit edges: worst %.3f sample from a true one; protect_m %.0f m' % (np.abs(ee).max(), fix.protect_m))
    assert np.abs(ee).max() <= 0.25                  # ('track': the edge is the code start itself)
    assert fix.ok and len(fix.prns) == 8
    assert err <= bound('strong', None, 'track', fix.g)
    k = int(np.flatnonzero(meas['prn'] == fix.ref_prn)[0])
    assert fix.sample == meas['sample'][k] and abs(fix.t_gps - T.t_gps_of(info, fix.sample)) < 0.1
    # the same from an a-priori at the edge of the contract
    far = T.TRUTH + 50.0e3 * np.array([0.6, 0.0, 0.8])
    fix2 = S.coarse_time_fix(meas, info['ephs'], T.t_gps_of(info, fix.sample) - 30.0, far)
    assert fix2.ok and np.linalg.norm(fix2.ecef - fix.ecef) <= 1.0e-3


def test_mixed_scene_uses_the_weak_satellites(acqs):
    from gpsmi.pipeline import Receiver
    sc, info = T.mixed()
    data = T.c64('mixed')
    fix, meas, ms = S.snapshot_fix(acqs[0], data, info['ephs'], info['t0_gps'] + TIME_OFF)
    err, pe, fe = report('mixed', sc, fix, meas, ms, len(data))
    assert meas['prn'].tolist() == sorted(info['ephs']) and len(meas) == 6
    assert fix.ok and set(T.MIXED_WEAK) <= set(fix.prns) and len(fix.prns) == 6
    assert fix.dropped == [] and np.isfinite(fix.protect_m)      # (six satellites: nothing may be dropped)
    assert err <= bound('mixed', None, 'track', fix.g)
    # a plain receiver on the same data: no subframe, no fix
    rx = Receiver()
    solver = S.P.PositionSolver(ephemerides=info['ephs'])
    fixes = []
    try:
        for b in range(len(data) // 65536):
            rx.feed(data[b * 65536:(b + 1) * 65536])
        rx.drain()
        for dg in rx.result_list:
            fixes += solver.feed(pickle.loads(dg))
        tracked = set(rx.act_sat_set)
    finally:
        rx.close()
    print('plain receiver: tracks %s, %d datagrams, %d fixes' % (sorted(tracked), len(rx.result_list), len(fixes)))
    assert fixes == [] and not tracked & set(T.MIXED_WEAK)


def test_two_blocks(acqs):
    sc, info = T.strong()
    raw = T.raw('strong')[:T.TWO_BLOCKS]
    fix, meas, ms = S.snapshot_fix(acqs[1], raw, info['ephs'], info['t0_gps'] + TIME_OFF, source='refine')
    err, pe, fe = report('two blocks', sc, fix, meas, ms, len(raw))
    assert meas['prn'].tolist() == [2, 5, 8, 10, 13, 16, 19, 21]
    assert (meas['sample'] == 0).all() and {s.decode() for s in meas['source']} == {'refine'}
    assert fix.ok and err <= bound('strong', T.TWO_BLOCKS, 'refine', fix.g)
    assert np.isnan(meas['edge']).all()              # (60 ms: two bits do not place an edge)
    # the default source is refinement where tracking does not apply
    again = S.measure(acqs[1], raw, prns=sorted(info['ephs']))
    assert again.tobytes() == meas.tobytes()
    # the shortest snapshot: 40 ms of refinement and the code slide
    short = S.measure(acqs[1], raw[:S.min_samples(2048)], prns=sorted(info['ephs']))
    pe = T.phase_error(sc, short)
    print('86017 samples: %d measured, code phase errors %s' % (len(short), np.round(pe, 3)))
    assert short['prn'].tolist() == [2, 5, 8, 10, 13, 16, 19, 21]
    with pytest.raises(ValueError):
        S.measure(acqs[1], raw[:S.min_samples(2048) - 1], prns=sorted(info['ephs']))


def test_same_bytes_from_every_input(acqs):
    from gpsmi.engine import DeviceBuffer
    _, info = T.strong()
    prns = sorted(info['ephs'])
    raw, c64 = np.ascontiguousarray(T.raw('strong')), T.c64('strong')
    ref = S.measure(acqs[0], c64, prns=prns)
    assert len(ref) == 8
    assert S.measure(acqs[0], c64, prns=prns).tobytes() == ref.tobytes()
    assert S.measure(acqs[1], raw, prns=prns).tobytes() == ref.tobytes()
    for acq, arr in ((acqs[0], c64), (acqs[1], raw)):
        buf = DeviceBuffer(arr.nbytes)
        try:
            buf.upload(arr)
            assert S.measure(acq, (buf.ptr, len(arr)), prns=prns).tobytes() == ref.tobytes()
        finally:
            buf.free()


def test_absent_prn_is_not_measured(acqs):
    _, info = T.strong()
    ephs = dict(info['ephs'])
    ephs[27] = dict(ephs[2])                          # an ephemeris for a satellite that is not there
    stats = {}
    meas = S.measure(acqs[1], T.raw('strong'), prns=sorted(ephs), stats=stats)
    print('searched %s, hits over the threshold %s' % (sorted(ephs), [(h[1], round(h[0], 1)) for h in stats['found']]))
    assert meas['prn'].tolist() == [2, 5, 8, 10, 13, 16, 19, 21]
