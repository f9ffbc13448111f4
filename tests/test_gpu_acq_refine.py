"""GPU: the refinement of weak / deep hits (gpsmi_acq_refine / AcqEngine.refine /
Acquisition.refineHits) against the float64 restatement (refine_ref.py) and the truth of the pinned
deep scene, the equivalence of its inputs, the 16368 configuration, and the path from the deep
search through refineHits and hit_at, down to tools/run_file.py --deep-acq --refine.

Tolerances against the restatement: the GPU works in float32 and takes its carrier from 24 bits of
an integer phase, so they were measured on the first GPU run (the largest deviation over cases A
and B, six candidates each; 16368 on its own) and are asserted at four times that; the measured
values stand beside each constant and in DESIGN.md 4.2f."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from deep_ref import DEEP_HIGH, DEEP_N_COH, DEEP_N_SEG, DEEP_ZERO, L1_HZ, deep_scene, nearest_bin
from refine_ref import check_truth, refine_ref, scene_cases
from test_gpu_acq_noncoherent import CFG, _engine, _same, _upload

pytestmark = pytest.mark.gpu

N_MS = 1000
N_BLOCKS = 33

# asserted = 4 x the largest deviation measured on the first GPU run (MI355X; cases A and B at 2048,
# the 300-ms case at 16368)                               measured
TOL = {2048: dict(prompts=4 * 2.825e-07,     # / max|P|      2.625e-07 (A), 2.825e-07 (B)
                  grid=4 * 1.768e-07,        # / peak        1.768e-07 (A), 1.728e-07 (B)
                  f_hz=4 * 3.653e-05,        # Hz            3.328e-05 (A), 3.653e-05 (B)
                  mu=4 * 6.407e-07,          # absolute      6.407e-07 (A), 4.260e-07 (B)
                  code_phase=4 * 9.178e-08), # samples       9.178e-08 (A), 6.365e-08 (B)
       16368: dict(prompts=4 * 2.678e-07, grid=4 * 2.952e-07, f_hz=4 * 1.804e-05, mu=4 * 1.376e-06,
                   code_phase=4 * 2.846e-07)}
PROMPT_CAP = 1e-3                            # the tracker's correlator I/Q is held to this
assert all(t['prompts'] <= PROMPT_CAP for t in TOL.values())


@pytest.fixture(scope='module')
def scene_raw():
    return deep_scene().block_raw(0, n=N_BLOCKS * 65536)


@pytest.fixture(scope='module')
def scene_c64(scene_raw):
    from gpsmi.synth import raw_to_c64
    return raw_to_c64(scene_raw)


def deviations(rec, grid, P, ref, rgrid, rP):
    """The largest deviations of a call from the restatement, as the tolerances count them."""
    dev = dict(prompts=0.0, grid=0.0, f_hz=0.0, mu=0.0, code_phase=0.0)
    for h in range(len(rec)):
        dev['prompts'] = max(dev['prompts'], np.abs(P[h] - rP[h]).max() / np.abs(rP[h]).max())
        dev['grid'] = max(dev['grid'], np.abs(grid[h] - rgrid[h]).max() / ref['peak'][h])
    dev['f_hz'] = np.abs(rec['f_hz'] - ref['f_hz']).max()
    dev['mu'] = np.abs(rec['mu'] - ref['mu']).max()
    dev['code_phase'] = np.abs(rec['code_phase'] - ref['code_phase']).max()
    return dev


def check_numbers(dev, cs, what):
    print('deviations %s cs %d: ' % (what, cs) + '  '.join('%s %.3e' % kv for kv in dev.items()))
    for k, v in dev.items():
        assert v <= TOL[cs][k], (k, v, TOL[cs][k])


# ---- 1, 2. decisions and numbers at 2048 ----------------------------------------------------------

@pytest.mark.parametrize('case', ['A', 'B'])
def test_decisions_and_numbers(scene_c64, case):
    first, hits, truth = scene_cases(deep_scene(), N_MS, 2048)[case]
    data = scene_c64[first:]
    ref, rgrid, rP = refine_ref(data, hits, N_MS, 2048)
    e = _engine(2048)
    try:
        rec, grid, P = e.refine(data, hits, N_MS, want_grid=True, want_prompts=True)
        assert e.last_ms() > 0
    finally:
        e.close()
    assert np.array_equal(rec['prn'], ref['prn']) and np.all(rec['n_bits'] == 49)
    assert np.array_equal(rec['edge_ms'], ref['edge_ms'])
    assert np.array_equal(rec['confirmed'], ref['confirmed'])
    check_truth(rec, truth)
    check_numbers(deviations(rec, grid, P, ref, rgrid, rP), 2048, 'case ' + case)


# ---- 3. input equivalence ------------------------------------------------------------------------------

def test_same_bytes_from_every_input(scene_raw, scene_c64):
    """complex64 and raw u8, host and device input; one hit alone and among six; two calls."""
    _, hits, _ = scene_cases(deep_scene(), N_MS, 2048)['A']
    e, er = _engine(2048), _engine(2048, raw_u8=True)
    bufs = []
    try:
        rec, grid, P = e.refine(scene_c64, hits, N_MS, want_grid=True, want_prompts=True)
        again = e.refine(scene_c64, hits, N_MS, want_grid=True, want_prompts=True)
        for a, b in zip((rec, grid, P), again):
            _same(a, b)
        raw = er.refine(scene_raw, hits, N_MS, want_grid=True, want_prompts=True)
        for a, b in zip((rec, grid, P), raw):
            _same(a, b)
        for eng, arr in ((e, scene_c64), (er, scene_raw)):
            bufs.append(_upload(arr))
            dev = eng.refine((bufs[-1].ptr, len(arr)), hits, N_MS, want_grid=True, want_prompts=True)
            for a, b in zip((rec, grid, P), dev):
                _same(a, b)
        for h in (0, 3, 5):
            one, g1, p1 = e.refine(scene_c64, [hits[h]], N_MS, want_grid=True, want_prompts=True)
            _same(one, rec[h:h + 1])
            _same(g1, grid[h:h + 1])
            _same(p1, P[h:h + 1])
        rev = e.refine(scene_c64, hits[::-1], N_MS)
        _same(rev[::-1], rec)
    finally:
        for b in bufs:
            b.free()
        e.close()
        er.close()


def test_hit_near_sample_zero_takes_the_next_period(scene_c64):
    """delay < tap: the windows start one code period later, nothing is read before sample 0."""
    s = deep_scene().sats[0]
    cut = int(s.delay)
    hit = [(s.prn, nearest_bin(s.doppler), 0)]
    ref, _, rP = refine_ref(scene_c64[cut:], hit, N_MS, 2048)
    e = _engine(2048)
    try:
        rec, P = e.refine(scene_c64[cut:], hit, N_MS, want_prompts=True)
    finally:
        e.close()
    dp = np.abs(P - rP).max() / np.abs(rP).max()
    print('prompts %.3e  f_hz %.3e  code_phase %.3e' % (dp, abs(rec['f_hz'][0] - ref['f_hz'][0]),
                                                       abs(rec['code_phase'][0] - ref['code_phase'][0])))
    assert rec['edge_ms'][0] == ref['edge_ms'][0] == 19 and rec['confirmed'][0] == 1
    assert dp <= TOL[2048]['prompts']
    assert abs(rec['f_hz'][0] - ref['f_hz'][0]) <= TOL[2048]['f_hz']


# ---- 4. 16368 / N_CYC 8 ---------------------------------------------------------------------------------

def test_hirate_300_ms():
    """deep_scene(16368, 8), 300 ms, early / late at 8 samples.  Satellites whose true edge the
    restatement itself does not find over this span are left out (and printed); at least three of
    the five must remain."""
    cs, n_ms = 16368, 300
    sc = deep_scene(cs, 8)
    data = sc.block(0, n=(n_ms + 2) * cs + 8)
    _, hits, truth = scene_cases(sc, n_ms, cs)['A']
    ref, rgrid, rP = refine_ref(data, hits, n_ms, cs, tap=8)
    keep = [h for h in range(5) if ref['edge_ms'][h] == truth[h][2]]
    print('left out:', [hits[h][0] for h in range(5) if h not in keep])
    assert len(keep) >= 3
    e = _engine(cs)
    try:
        rec, grid, P = e.refine(data, hits, n_ms, tap_samples=8, want_grid=True, want_prompts=True)
        dflt = e.refine(data, hits, n_ms)                 # 8 is the default at 16368
    finally:
        e.close()
    _same(dflt, rec)
    for h in range(6):
        print(h, rec[h], ref[h]['edge_ms'], ref[h]['ratio'], ref[h]['f_hz'], ref[h]['code_phase'])
    sel = keep + [5]
    assert np.array_equal(rec['edge_ms'][sel], ref['edge_ms'][sel])
    assert np.array_equal(rec['confirmed'][sel], ref['confirmed'][sel])
    dev = deviations(rec[sel], grid[sel], P[sel], ref[sel], rgrid[sel], rP[sel])
    check_numbers(dev, cs, '300 ms')


# ---- 5. end to end -----------------------------------------------------------------------------------------

GRID = [-5000.0 + 200.0 * i for i in range(51)]


def test_deep_search_to_refined_hits(scene_c64):
    """sweepDeepSats -> refineHits -> hit_at: five confirmed records whose delay one second on is
    within one sample of synth's truth."""
    from gpsmi.acquisition import Acquisition, hit_at
    acq = Acquisition()
    try:
        found = []
        res = acq.sweepDeepSats(scene_c64[:DEEP_N_SEG * DEEP_N_COH * 2048], GRID, list(range(2, 33)),
                                found, n_coh=DEEP_N_COH, n_seg=DEEP_N_SEG)
        rec = acq.refineHits(scene_c64, res)
        assert rec['n_bits'][0] == 1040 // 20 - 1          # 33 blocks hold 1056 ms: n_ms 1040
        truth = {p: (f, d) for p, f, d in DEEP_HIGH + [DEEP_ZERO]}
        assert sorted(rec['prn'].tolist()) == sorted(truth) and [r[1] for r in res] == rec['prn'].tolist()
        sample = 2048000
        for r in rec:
            dop, delay = truth[int(r['prn'])]
            f, d = hit_at(r, sample, acq.cfg)
            true = (delay - dop / L1_HZ * sample) % 2048
            print(r, d, true)
            assert r['confirmed'] == 1 and abs(f - dop) <= 6.0
            assert min((d - true) % 2048, (true - d) % 2048) <= 1.0
    finally:
        acq.engine.close()


def test_noise_alone_confirms_nothing():
    """The same scene with every amplitude 0 (same seed): the largest cell of the deep search for
    three PRNs, whatever it is, is not confirmed."""
    from gpsmi.acquisition import Acquisition, norm_max_corr
    noise = deep_scene(amp=0.0).block(0, n=N_BLOCKS * 65536)
    acq = Acquisition()
    try:
        prns = [6, 10, 29]
        tab = acq.engine.search_deep(noise[:DEEP_N_SEG * DEEP_N_COH * 2048], prns, GRID, DEEP_N_COH,
                                     DEEP_N_SEG)
        cand = []
        for j, p in enumerate(prns):
            nmc = [norm_max_corr(tab[b, j]) for b in range(len(GRID))]
            b = int(np.argmax(nmc))
            cand.append((nmc[b], p, GRID[b], int(tab[b, j]['argmax'])))
        rec = acq.refineHits(noise, cand, n_ms=N_MS)
        print(cand, rec)
        assert not rec['confirmed'].any()
    finally:
        acq.engine.close()


# ---- 6. command line -------------------------------------------------------------------------------------

def test_run_file_refine(tmp_path, scene_raw):
    from conftest import ROOT
    path = tmp_path / 'deep.bin'
    scene_raw.tofile(path)
    base = [sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), str(path), '--seconds', '0.3',
            '--deep-acq', '1.0']
    r = subprocess.run(base + ['--refine', '--json'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])['deep_acquisition']
    truth = {p: (f, dl) for p, f, dl in DEEP_HIGH + [DEEP_ZERO]}
    recs = d['refined']['records']
    assert sorted(q['prn'] for q in recs) == sorted(truth) and d['refined']['device_ms'] > 0
    for q in recs:
        dop, delay = truth[q['prn']]
        assert q['confirmed'] and q['edge_ms'] == 0 and abs(q['f_hz'] - dop) <= 6.0
        assert abs(q['code_phase'] - delay) <= 0.5 and 22.0 <= q['cn0_dbhz'] <= 26.0
    r = subprocess.run(base + ['--refine'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for p in truth:
        assert any(line.split()[:2] == ['PRN', str(p)] and 'f_hz' in line and 'edge_ms' in line
                   and 'code_phase' in line and 'cn0_dbhz' in line and 'ratio' in line
                   and 'confirmed True' in line for line in r.stdout.splitlines()), r.stdout
    r = subprocess.run(base + ['--json'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])['deep_acquisition']
    assert sorted(d) == ['device_ms', 'found', 'n_coh', 'n_seg', 'searched', 'seconds']


# ---- what is refused --------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_usable(scene_c64):
    from gpsmi.engine import AcqEngine, Config, EngineError
    _, hits, _ = scene_cases(deep_scene(), N_MS, 2048)['A']
    e = _engine(2048)
    try:
        ok = e.refine(scene_c64, hits[:2], 100)
        for kw, code in ((dict(n_ms=90), 1), (dict(n_ms=100, df_step=0.1), 1), (dict(n_ms=2000), 1),
                         (dict(n_ms=100, carrier_hz=float('nan')), 1)):
            with pytest.raises(EngineError, match=r'\(-%d\)' % code):
                e.refine(scene_c64, hits[:2], **kw)
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.refine(scene_c64, hits * 11, 100)
        _same(e.refine(scene_c64, hits[:2], 100), ok)
    finally:
        e.close()
    e = AcqEngine(Config(code_samples=4096, n_cyc=8))
    try:
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.refine(np.zeros(50 * 4096, np.complex64), [(6, 0.0, 10)], 40)
    finally:
        e.close()
