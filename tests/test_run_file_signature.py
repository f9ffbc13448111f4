"""tools/run_file.py --antenna FILE ... with --snapshot S --spoof-check: the
argument rules -- legal there without --null, refused without --spoof-check, with --null, with a
conditioning stage or a foreign format; the streaming run still wants --null -- and, on the GPU, the
verdict in the report of the four-antenna spoofed scene."""
import json

import numpy as np
import pytest

import snapshot_truth as T
import spoof_truth as ST
from test_run_file_spoof import run_file


@pytest.fixture()
def files(tmp_path):
    out = []
    for k in range(3):
        p = str(tmp_path / f'ant{k}.bin')
        open(p, 'wb').close()
        out.append(p)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in T.strong()[1]['ephs'].items()}, f)
    return out, eph


def snap(eph):
    return ['--snapshot', '1.0', '--ephemeris', eph, '--time', '100000.0']


def test_antenna_rules_with_snapshot(files):
    (a0, a1, a2), eph = files
    more = ['--antenna', a1, '--antenna', a2]
    for extra, word in ((more, '--spoof-check'),                                   # the signatures serve the check
                        (more + ['--spoof-check', '--null'], '--null'),
                        (more + ['--spoof-check', '--null-taps', '3'], '--null'),
                        (more + ['--spoof-check', '--excise'], '--excise'),
                        (more + ['--spoof-check', '--blank'], '--blank'),
                        (more + ['--spoof-check', '--format', 'sc16'], 'own format'),
                        (['--antenna', a1] * 8 + ['--spoof-check'], 'seven')):
        r = run_file(a0, *snap(eph), *extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr[-500:])
    # legal: the call gets as far as reading the (empty) files
    r = run_file(a0, *snap(eph), *more, '--spoof-check')
    assert r.returncode != 2 and 'the recording holds 0 samples' in r.stderr, r.stderr[-500:]


def test_streaming_run_still_wants_null(files):
    (a0, a1, _), _ = files
    r = run_file(a0, '--antenna', a1)
    assert r.returncode == 2 and '--null go together' in r.stderr
    r = run_file(a0, '--null')
    assert r.returncode == 2 and '--null go together' in r.stderr
    r = run_file(a0, '--antenna', a1, '--spoof-check')
    assert r.returncode == 2


@pytest.mark.gpu
def test_verdict_is_printed(tmp_path):
    import sig_ref as R
    from gpsmi import position as P
    sc, info, _ = ST.spoofed()
    arr = R.snapshot_array('spoofed')
    rows = R.snapshot_raw('spoofed')
    tail = arr.block_raw(31)[:, rows.shape[1] - 31 * 65536:]                  # (the reader takes whole blocks)
    paths = []
    for a in range(R.SNAP_ANTENNAS):
        paths.append(str(tmp_path / f'ant{a}.bin'))
        with open(paths[-1], 'wb') as f:
            rows[a].astype('<u2').tofile(f)
            tail[a].astype('<u2').tofile(f)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    lat, lon, h = (float(v) for v in P.ecef_to_geo(ST.spoofer_pos() + 100.0))
    common = [paths[0], '--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + ST.TIME_OFF),
              '--near', f'{lat!r},{lon!r},{h!r}', '--spoof-check']
    for p in paths[1:]:
        common += ['--antenna', p]
    r = run_file(*common, '--json')
    assert r.returncode == 0, r.stderr[-2000:]
    sp = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']['spoof']
    assert sp['antennas'] == 4 and sp['authentic'] == 0 and sp['one_source'] == [False, True] and not sp['one_direction']
    assert sp['alarm'] and sp['signature_ms'] > 0 and len(sp['fixes']) == 2
    for fx, pos in zip(sp['fixes'], (T.TRUTH, ST.spoofer_pos())):             # the authentic fix first
        assert fx['ok'] and np.linalg.norm(np.array(fx['ecef_m']) - pos) < 100.0
    r = run_file(*common)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    assert 'fix a is authentic' in r.stdout and 'one direction for every signal over 4 antennas: no' in r.stdout
