"""tools/run_file.py --snapshot S --cancel [DBHZ]: the flag is passed through to
snapshot.measure, refused without --snapshot, and without it the output is what it was."""
import json
import os
import subprocess
import sys

import pytest

import snapshot_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_file(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), *args], capture_output=True,
                          text=True, timeout=300)


def test_cancel_needs_snapshot(tmp_path):
    path = str(tmp_path / 'empty.bin')
    open(path, 'wb').close()
    for extra in (['--cancel'], ['--cancel', '45']):
        r = run_file(path, *extra)
        assert r.returncode == 2 and '--cancel needs --snapshot' in r.stderr


@pytest.mark.gpu
def test_cancel_is_passed_through(tmp_path):
    sc, info = T.strong()
    path = str(tmp_path / 'second.bin')
    with open(path, 'wb') as f:
        T.raw('strong').astype('<u2').tofile(f)
        sc.block_raw(31)[len(T.raw('strong')) - 31 * 65536:].astype('<u2').tofile(f)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    common = [path, '--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + 20.0)]
    outs = {}
    for name, extra in (('plain', ['--json']), ('cancel', ['--cancel', '--json'])):
        r = run_file(*common, *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = r.stdout
    plain = json.loads(outs['plain'].strip().splitlines()[-1])['snapshot']
    canc = json.loads(outs['cancel'].strip().splitlines()[-1])['snapshot']
    assert 'cancelled' not in plain and plain['ok']
    # every satellite of this scene is above 40 dB-Hz: all are cancelled, and measured as before
    assert sorted(c['prn'] for c in canc['cancelled']) == [2, 5, 8, 10, 13, 16, 19, 21]
    assert all(0.0 < c['removed'] < 0.2 and c['n_skipped'] <= 2 for c in canc['cancelled'])
    assert canc['measurements'] == plain['measurements'] and canc['ok']
    assert canc['position'] == plain['position']
    # a threshold of its own, between the fourth and the fifth reading; the text form
    cn0 = sorted(m['cn0_dbhz'] for m in plain['measurements'])
    thr = 0.5 * (cn0[3] + cn0[4])
    r = run_file(*common, '--cancel', repr(thr))
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert r.stdout.count('cancelled PRN') == sum(c >= thr for c in cn0)
