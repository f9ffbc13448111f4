"""tools/run_file.py --snapshot: the 1-s strong scene of snapshot_truth.py written as a recording,
a fix from its first second with stored ephemerides and a time 20 s off, within
the bound of tests/test_gpu_snapshot.py; and the command's output without the new flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TODAY = {'file', 'blocks', 'signal_s', 'wall_s', 'x_realtime', 'acquired', 'tracked', 'datagrams', 'fixes',
         'ephemerides_decoded'}                       # (a second of signal: no 'position')


def run_file(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), *args], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.gpu
def test_snapshot_of_a_recording(tmp_path):
    sc, info = T.strong()
    path = str(tmp_path / 'second.bin')
    with open(path, 'wb') as f:                       # 32 whole blocks: the second and 48 ms more
        T.raw('strong').astype('<u2').tofile(f)
        sc.block_raw(31)[len(T.raw('strong')) - 31 * 65536:].astype('<u2').tofile(f)
    assert os.path.getsize(path) == 32 * 65536 * 2
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    out = json.loads(run_file(path, '--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + 20.0),
                              '--json').strip().splitlines()[-1])
    assert set(out) == {'file', 'snapshot'}
    s = out['snapshot']
    err = float(np.linalg.norm(np.array(s['position']['ecef_m']) - T.TRUTH)) if s['ok'] else float('nan')
    print('snapshot: ok %s %s, %.2f m from the truth, g %s, %s ms on the device, %d measurements' % (
        s['ok'], s['reason'], err, s.get('g'), s['device_ms'], len(s['measurements'])))
    assert s['ok'] and s['seconds'] == 1.0 and s['device_ms'] > 0
    assert [m['prn'] for m in s['measurements']] == s['satellites'] == [2, 5, 8, 10, 13, 16, 19, 21]
    ref_err, ref_g = T.REF['strong', None, 'track']
    assert abs(s['g'] - ref_g) <= 0.01 * ref_g
    assert err <= min(2.0 * ref_err, s['g'] * 0.25 * 299792458.0 / 2048000.0)
    assert abs(s['position']['lat_deg'] - 49.082961) < 1e-3 and abs(s['position']['lon_deg'] - 8.307581) < 1e-3
    # the text form, with a position as far as known, a UTC time and both filters in the way
    txt = run_file(path, '--snapshot', '0.5', '--ephemeris', eph, '--time', '2024-10-30T11:19:21Z', '--near', '49.3,8.6',
                   '--excise', '--blank')
    assert 'fix from 8 satellites' in txt and 'PRN 21' in txt
    # without the new flags: today's keys
    plain = json.loads(run_file(path, '--ephemeris', eph, '--json').strip().splitlines()[-1])
    assert set(plain) == TODAY
