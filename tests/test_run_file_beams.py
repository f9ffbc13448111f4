"""tools/run_file.py --snapshot S --spoof-check --antenna FILE ... --beams: the
argument rules, and on the GPU the per-record lines of the four-antenna spoofed scene."""
import json
import re

import pytest

import spoof_truth as ST
from test_run_file_signature import files, snap  # noqa: F401  (the fixture of empty files)
from test_run_file_spoof import run_file


def test_beams_rules(files):  # noqa: F811
    (a0, a1, a2), eph = files
    r = run_file(a0, *snap(eph), '--spoof-check', '--beams')
    assert r.returncode == 2 and '--beams needs --antenna' in r.stderr
    r = run_file(a0, '--antenna', a1, '--null', '--beams')
    assert r.returncode == 2 and '--beams needs --snapshot' in r.stderr
    # legal: the call gets as far as reading the (empty) files
    r = run_file(a0, *snap(eph), '--antenna', a1, '--antenna', a2, '--spoof-check', '--beams')
    assert r.returncode != 2 and 'the recording holds 0 samples' in r.stderr, r.stderr[-500:]


@pytest.mark.gpu
def test_beam_lines_are_printed(tmp_path):
    import sig_ref as R
    from gpsmi import position as P
    from test_beams import RESTATED
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
    lat, lon, h = (float(v) for v in P.ecef_to_geo(ST.apriori()))
    common = [paths[0], '--snapshot', '1.0', '--ephemeris', eph, '--time', repr(info['t0_gps'] + ST.TIME_OFF),
              '--near', f'{lat!r},{lon!r},{h!r}', '--spoof-check', '--beams']
    for p in paths[1:]:
        common += ['--antenna', p]
    r = run_file(*common)
    assert r.returncode == 0, r.stderr[-2000:]
    beams = re.findall(r'^  beam PRN +(\d+)  (null at the spoofer|no null) +gain +([-\d.]+) dB  flags \[1\]  '
                       r'cn0_dbhz on antenna 0 ([\d.]+)  measured on the beam$', r.stdout, re.M)
    meas = re.findall(r'^  PRN +(\d+)  sample .* cn0_dbhz ([\d.]+)  \((\w+)\)$', r.stdout, re.M)
    assert len(beams) == len(meas) == 16, r.stdout[-3000:]
    assert [int(b[0]) for b in beams] == [int(m[0]) for m in meas] == sorted(2 * sorted(RESTATED))
    # per PRN one record with the restated null or none (the authentic one) and one without (the added one)
    for prn, (carries, _, _) in RESTATED.items():
        assert sorted(b[1] == 'null at the spoofer' for b in beams if int(b[0]) == prn) == [False, bool(carries)]
    # the records were measured on the beams: tracked there, every C/N0 above its antenna-0 value
    assert all(m[2] == 'track' and float(m[1]) > float(b[3]) for m, b in zip(meas, beams))
    assert 'fix a is authentic' in r.stdout
