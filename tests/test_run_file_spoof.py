"""tools/run_file.py --snapshot S --spoof-check [K]: the flag is passed through to
snapshot_fix, refused without --snapshot, and prints the doubled PRNs, both fixes and their
separation on a synthetic recording; the exit status is 0 with and without an alarm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_truth as T
import spoof_truth as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_file(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), *args], capture_output=True,
                          text=True, timeout=300)


def test_spoof_check_needs_snapshot(tmp_path):
    path = str(tmp_path / 'empty.bin')
    open(path, 'wb').close()
    for extra in (['--spoof-check'], ['--spoof-check', '3']):
        r = run_file(path, *extra)
        assert r.returncode == 2 and '--spoof-check needs --snapshot' in r.stderr


def recording(tmp_path, name, sc, raw):
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        raw.astype('<u2').tofile(f)
        sc.block_raw(31)[len(raw) - 31 * 65536:].astype('<u2').tofile(f)      # (the reader takes whole blocks)
    return path


@pytest.mark.gpu
def test_spoof_check_prints_both_fixes(tmp_path):
    from gpsmi import position as P
    sc, info, _ = ST.spoofed()
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    lat, lon, h = (float(v) for v in P.ecef_to_geo(ST.apriori()))
    common = ['--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + ST.TIME_OFF),
              '--near', f'{lat!r},{lon!r},{h!r}', '--spoof-check']
    path = recording(tmp_path, 'spoofed.bin', sc, ST.raw())
    r = run_file(path, *common, '--json')
    assert r.returncode == 0, r.stderr[-2000:]
    sp = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']['spoof']
    assert sp['doubled'] == sorted(info['ephs']) and sp['alarm'] and len(sp['fixes']) == 2
    assert all(fx['ok'] for fx in sp['fixes']) and abs(sp['separation_m'] - ST.SPOOF_OFF_M) < 100.0
    for fx, pos in zip(sp['fixes'], (T.TRUTH, ST.spoofer_pos())):
        assert np.linalg.norm(np.array(fx['ecef_m']) - pos) < 100.0
    r = run_file(path, *common)                        # the text form
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert 'ALARM' in r.stdout and 'fix a:' in r.stdout and 'fix b:' in r.stdout and 'm apart' in r.stdout
    # the clean recording: no alarm, one fix, exit status 0; without the flag no 'spoof' entry
    clean = recording(tmp_path, 'clean.bin', T.strong()[0], T.raw('strong'))
    r = run_file(clean, *common, '--json')
    assert r.returncode == 0, r.stderr[-2000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']
    assert s['spoof']['doubled'] == [] and not s['spoof']['alarm'] and s['spoof']['separation_m'] is None and s['ok']
    r = run_file(clean, *common[:-1], '--json')
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']
    assert 'spoof' not in plain and plain['measurements'] == s['measurements'] and plain['position'] == s['position']
