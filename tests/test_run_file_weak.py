"""tools/run_file.py --weak-fix: the argument rules and, without the flag, a report
with exactly the keys it had (CPU: the receiver is a stand-in that acquires nothing, the file loop,
the solver and the report are the command's own)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['file', 'blocks', 'signal_s', 'wall_s', 'x_realtime', 'acquired', 'tracked', 'datagrams', 'fixes',
        'ephemerides_decoded']


def test_weak_fix_needs_track():
    tool = os.path.join(ROOT, 'tools', 'run_file.py')
    for extra in ([], ['--deep-acq', '1'], ['--deep-acq', '1', '--refine']):
        r = subprocess.run([sys.executable, tool, 'none.bin', '--weak-fix'] + extra, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and '--weak-fix needs --track' in r.stderr
    r = subprocess.run([sys.executable, tool, '--help'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and '--weak-fix' in r.stdout


class _Receiver:
    """pipeline.Receiver's surface as run_file.run uses it; it finishes its sweep and tracks nothing."""

    def __init__(self, cfg, **kw):
        self.cfg, self.result_list, self.act_sat_set, self.found_sats = cfg, [], set(), []
        self.sweep_all_freq, self.n = True, 0

    def feed(self, data, skip=0):
        self.n += 1
        self.sweep_all_freq = self.n < 3

    def drain(self):
        pass

    def close(self):
        pass


def test_report_keys_without_the_flag(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_file
    from gpsmi import pipeline
    monkeypatch.setattr(pipeline, 'Receiver', _Receiver)
    path = str(tmp_path / 'rec.bin')
    np.zeros(5 * 65536, '<u2').tofile(path)
    out = run_file.run(path)
    assert list(out) == KEYS and out['blocks'] == 5 and out['fixes'] == 0
    assert 'weak_fix' in run_file.run.__code__.co_varnames


import pytest  # noqa: E402


@pytest.mark.gpu
def test_weak_fix_on_the_mixed_recording(tmp_path):
    """The mixed scene of test_gpu_weaknav.py as a recording: three satellites give no fix, with
    --weak-fix the three lowered ones are merged in and the fix holds the bounds set there."""
    import json
    import weaknav_scene as S
    from test_gpu_weaknav import CAP_MEAN_M, FIX_MEAN_M
    sc, info, low = S.mixed()
    path = str(tmp_path / 'mixed.bin')
    with open(path, 'wb') as f:
        for b in range(S.MIXED_BLOCKS):
            sc.block_raw(b).astype('<u2').tofile(f)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    base = [sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path, '--ephemeris', eph, '--json',
            '--deep-acq', '1', '--refine', '--track']
    r = subprocess.run(base + ['--weak-fix'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out['weak_fix'], out['fixes'], out.get('position'))
    assert list(out)[:len(KEYS)] == KEYS and len(out['tracked']) == 3
    w = out['weak_fix']['channels']
    assert sorted(q['prn'] for q in w) == low
    assert all(q['subframes'] >= 1 and q['fixes'] == out['fixes'] for q in w) and out['fixes'] > 30
    err = np.linalg.norm(np.array(out['position']['ecef_m']) - S.TRUTH)
    assert err <= min(2.0 * FIX_MEAN_M, CAP_MEAN_M)
