"""GPU, end to end: gpsmi.snapshot with array=True on the scene of tests/array_truth.py -- eight
satellites at about 20.5 dB-Hz over four antennas, one second.  Antenna 0 alone measures fewer than five
of them and has no fix; the array search finds all eight, every one is measured on a beam of its own,
and the fix follows.

The reference is the same scene rendered 6.02 dB stronger (the amplitude doubled: 10 log10 4 = 6.0 dB
is what four coherent antennas can give) and measured on antenna 0 alone, in the same test run: every
code phase of the array lies within twice its worst code-phase error, the fix within twice its
distance from the truth.  The figures of an MI355X run are in DESIGN.md 4.2s."""
import json

import numpy as np
import pytest

import array_truth as AT
import snapshot_truth as T
from gpsmi import snapshot as S

pytestmark = pytest.mark.gpu

TIME_OFF = 20.0
PRNS = [2, 5, 8, 10, 13, 16, 19, 21]


@pytest.fixture(scope='module')
def acq():
    from gpsmi.acquisition import Acquisition
    a = Acquisition(raw_u8=True)
    yield a
    a.engine.close()


@pytest.fixture(scope='module')
def reference(acq):
    """(worst |code phase error| in samples, fix distance in m) of the 6 dB stronger scene on antenna 0."""
    arr, info = AT.scene(AT.REFERENCE_DB)
    fix, meas, ms = S.snapshot_fix(acq, np.ascontiguousarray(AT.raw(AT.REFERENCE_DB)[0]), info['ephs'],
                                   info['t0_gps'] + TIME_OFF)
    pe = T.phase_error(arr.scene, meas)
    assert meas['prn'].tolist() == PRNS and fix.ok, (meas['prn'].tolist(), fix.reason)
    err = float(np.linalg.norm(fix.ecef - T.TRUTH))
    print('\nreference (+6.02 dB, antenna 0 alone): code phase errors %s, fix %.2f m from the truth, cn0 %s' % (
        np.round(pe, 3), err, np.round(meas['cn0_dbhz'], 1)))
    return float(np.abs(pe).max()), err


def test_antenna_0_alone_has_no_fix(acq):
    arr, info = AT.scene()
    row0 = np.ascontiguousarray(AT.raw()[0])
    meas = S.measure(acq, row0, prns=sorted(info['ephs']))
    print('\nantenna 0 alone measures PRNs', meas['prn'].tolist())
    assert len(meas) < 5
    fix, _, _ = S.snapshot_fix(acq, row0, info['ephs'], info['t0_gps'] + TIME_OFF)
    assert not fix.ok


def test_array_finds_and_measures_all_eight(acq, reference):
    arr, info = AT.scene()
    stats = {}
    fix, meas, ms = S.snapshot_fix(acq, AT.raw(), info['ephs'], info['t0_gps'] + TIME_OFF, antennas=4, array=True,
                                   stats=stats)
    print('\narray hits', [(h[1], round(h[0], 1), h[2], h[3]) for h in stats['hits']])
    print('beams', [(b['prn'], b['kept'], round(b['gain_db'], 2)) for b in stats['beams']])
    print('device ms: array %.2f, signatures %.2f, beams %.2f, all %.2f' % (
        stats['array_ms'], stats['signature_ms'], stats['beams_ms'], ms))
    assert stats['array_ms'] > 0 and stats['signature_ms'] > 0 and stats['beams_ms'] > 0
    assert sorted(h[1] for h in stats['hits']) == PRNS
    assert meas['prn'].tolist() == PRNS
    pe = T.phase_error(arr.scene, meas)
    err = float(np.linalg.norm(fix.ecef - T.TRUTH)) if fix.ok else float('nan')
    print('array: code phase errors %s (reference worst %.3f), fix %s %.2f m from the truth (reference %.2f m), cn0 %s' % (
        np.round(pe, 3), reference[0], fix.ok or fix.reason, err, reference[1], np.round(meas['cn0_dbhz'], 1)))
    assert np.abs(pe).max() <= 2.0 * reference[0]
    assert fix.ok and err <= 2.0 * reference[1]
    # the same records from measure itself, from device-resident rows
    from gpsmi.engine import DeviceBuffer
    raw = AT.raw()
    buf = DeviceBuffer(raw.nbytes)
    try:
        buf.upload(raw)
        again = S.measure(acq, (buf.ptr, raw.shape[1]), prns=sorted(info['ephs']), antennas=4, array=True)
    finally:
        buf.free()
    assert again.tobytes() == meas.tobytes()


def test_sweep_array_sats_and_hits(acq):
    """Acquisition.sweepArraySats and pipeline.array_peak_hits on the scene: the eight satellites, the
    hit format of sweepDeepSats, the delays within one sample of the truth at the nearest bin."""
    from deep_ref import nearest_bin
    from gpsmi.pipeline import array_peak_hits
    arr, info = AT.scene()
    grid = [-5000.0 + 200.0 * i for i in range(51)]
    truth = AT.true_lags(arr.scene)
    hits = array_peak_hits(acq, AT.raw(), 4, list(range(2, 33)), grid, AT.N_COH, AT.N_SEG, corr_min=acq.cfg.corr_min)
    print('\narray_peak_hits', [(h[1], round(h[0], 1), h[2], h[3]) for h in hits])
    assert sorted(h[1] for h in hits) == PRNS
    for nmc, prn, f, d in hits:
        assert f == nearest_bin(truth[prn][0]) and abs(d - truth[prn][1]) <= 1 and nmc > acq.cfg.corr_min + 1
    lst, found = list(range(2, 33)), []
    res = acq.sweepArraySats(AT.raw(), 4, grid, lst, found, n_coh=AT.N_COH, n_seg=AT.N_SEG)
    assert res == sorted(found, reverse=True) and {s for _, s, _, _ in res} == set(PRNS)
    assert not set(lst) & set(PRNS)
    lst0, found0 = list(range(2, 33)), []
    res0 = acq.sweepDeepSats(np.ascontiguousarray(AT.raw()[0]), grid, lst0, found0, n_coh=AT.N_COH, n_seg=AT.N_SEG)
    print('sweepDeepSats on antenna 0:', res0)
    assert len(res0) < 5


def test_run_file_array_search(tmp_path):
    """tools/run_file.py --snapshot --antenna FILE --array-search on 128 ms of the strong scene over two
    antennas (four whole blocks a file)."""
    import os
    import subprocess
    import sys
    import sig_ref as SR
    from conftest import ROOT
    rows = SR.snapshot_raw('clean', 128)[:2]
    info = T.strong()[1]
    paths = []
    for a in range(2):
        paths.append(str(tmp_path / f'ant{a}.bin'))
        rows[a].astype('<u2').tofile(paths[-1])
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), paths[0], '--antenna', paths[1],
                        '--snapshot', '0.128', '--ephemeris', eph, '--time', repr(info['t0_gps'] + TIME_OFF),
                        '--array-search', '--json'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']
    a = s['array']
    assert a['antennas'] == 2 and a['array_ms'] > 0 and a['beams_ms'] > 0
    assert sorted(h['prn'] for h in a['hits']) == PRNS and a['antenna0_alone'] == PRNS
    assert [b['prn'] for b in a['beams'] if b['kept']] == [h['prn'] for h in a['hits']]
    assert [m['prn'] for m in s['measurements']] == PRNS and s['ok']
    err = float(np.linalg.norm(np.array(s['position']['ecef_m']) - T.TRUTH))
    print('\nrun_file --array-search: fix %.2f m from the truth, g %.3f' % (err, s['g']))
    assert err <= s['g'] * 0.25 * S.P.GPS_C / 2048000.0          # test_gpu_snapshot.py's bar: a quarter sample times g
