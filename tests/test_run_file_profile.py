"""tools/run_file.py --profile-check with --snapshot S --spoof-check: the argument
rules -- refused without --spoof-check and without --snapshot -- and, on the GPU, the report of the
lift-off second (liftoff_truth.py): one line per record, the distorted PRNs and the alarm."""
import json

import pytest

import liftoff_truth as LT
import snapshot_truth as T
import spoof_truth as ST
from test_run_file_spoof import run_file


@pytest.fixture()
def files(tmp_path):
    rec = str(tmp_path / 'rec.bin')
    open(rec, 'wb').close()
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in T.strong()[1]['ephs'].items()}, f)
    return rec, eph


def test_profile_check_rules(files):
    rec, eph = files
    snap = ['--snapshot', '1.0', '--ephemeris', eph, '--time', '100000.0']
    r = run_file(rec, '--profile-check')
    assert r.returncode == 2 and '--profile-check needs --snapshot' in r.stderr
    r = run_file(rec, *snap, '--profile-check')
    assert r.returncode == 2 and '--profile-check needs --spoof-check' in r.stderr
    # legal: the call gets as far as reading the (empty) file
    r = run_file(rec, *snap, '--spoof-check', '--profile-check')
    assert r.returncode != 2 and 'the recording holds 0 samples' in r.stderr, r.stderr[-500:]


@pytest.mark.gpu
def test_liftoff_is_reported(tmp_path):
    from gpsmi import position as P, snapshot as S
    sc, info, _ = LT.liftoff()
    raw = LT.raw()
    path = str(tmp_path / 'liftoff.bin')
    with open(path, 'wb') as f:
        raw.astype('<u2').tofile(f)
        sc.block_raw(31)[len(raw) - 31 * 65536:].astype('<u2').tofile(f)        # (the reader takes whole blocks)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    lat, lon, h = (float(v) for v in P.ecef_to_geo(ST.apriori()))
    common = [path, '--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + ST.TIME_OFF),
              '--near', f'{lat!r},{lon!r},{h!r}', '--spoof-check']
    r = run_file(*common, '--profile-check', '--json')
    assert r.returncode == 0, r.stderr[-2000:]
    sp = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']['spoof']
    assert sp['doubled'] == [] and sp['distorted'] == LT.REF_DISTORTED and sp['alarm']
    assert sp['profile_t_min'] == S.PROFILE_T_MIN and sp['profile_ms'] > 0 and len(sp['profile']) == 8
    assert sorted(f['prn'] for f in sp['profile'] if f['T'] > S.PROFILE_T_MIN) == LT.REF_DISTORTED
    r = run_file(*common, '--profile-check')
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert r.stdout.count('profile PRN') == 8 and r.stdout.count('DISTORTED') == len(LT.REF_DISTORTED)
    assert f'PRNs with a distorted profile {LT.REF_DISTORTED}; doubled or distorted: ALARM' in r.stdout
