"""GPU: bit-synchronous tracking of refined hits (gpsmi_acq_track / AcqEngine.track_weak /
Acquisition.trackHits) against the float64 restatement (wtrk_ref.py) and the truth of the pinned
deep scene, the equivalence of its inputs and of chunked calls, the 16368 configuration, data that
ends mid-span, and tools/run_file.py --deep-acq --refine --track.

Window starts.  Every n_k the GPU used -- floor(tau + k Tc) of the tau and f_hz its records carry --
is compared with the restatement's, for EVERY window.  (A scene none of whose 5400 window starts
lies within 1e-3 sample of an integer does not exist in practice: the sliding satellites cross an
integer five times a second in steps of 0.006 sample.  The guard is therefore put where it
belongs: test_acq_track.py asserts that the restatement's closest s_k, 5.7e-5 sample, is more than
1e-5 away, and the tau tolerance below is a hundred times smaller than that.)

Tolerances against the restatement: the GPU sums in float32, takes its carrier from 24 bits of an
integer phase and has its own libm, and the loops feed every deviation back; they were measured on
the first GPU run (the largest deviation over the weak and the strong scene, six channels, 45 bits;
16368 on its own) and are asserted at four times that; the measured values stand beside each
constant and in DESIGN.md 4.2g."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wtrk_ref as W
from deep_ref import DEEP_HIGH, DEEP_ZERO
from test_acq_track import F_RMS_BOUND, INTEGER_GUARD, check_truth
from test_gpu_acq_noncoherent import _engine, _same, _upload

pytestmark = pytest.mark.gpu

# asserted = 4 x the largest deviation measured on the first GPU run (MI355X)
#                                                  measured
TOL = {2048: dict(prompts=4 * 1.740e-06,   # / max|P|      1.740e-06 (weak), 7.124e-07 (strong)
                  f_hz=4 * 3.481e-06,      # Hz            3.481e-06 (weak), 1.808e-06 (strong)
                  tau=4 * 4.470e-08,       # samples       4.470e-08 (weak), 2.282e-08 (strong)
                  cn0=4 * 8.692e-06),      # dB            8.692e-06 (weak), 8.605e-06 (strong)
       16368: dict(prompts=4 * 3.107e-07, f_hz=4 * 1.174e-06, tau=4 * 2.068e-07, cn0=4 * 2.969e-06)}
PROMPT_CAP = 1e-3                            # the tracker's correlator I/Q is held to this
assert all(t['prompts'] <= PROMPT_CAP and t['tau'] <= INTEGER_GUARD / 10 for t in TOL.values())


def _cplx(rec, a):
    return rec[a + '_i'].astype(np.float64) + 1j * rec[a + '_q'].astype(np.float64)


def deviations(rec, ref):
    """The largest deviations of a call's records [nch, n_bits] from the restatement's."""
    dev = dict(prompts=0.0)
    for h in range(len(rec)):
        scale = np.abs(_cplx(ref[h], 'p')).max()
        for a in ('p', 'h0', 'h1'):
            dev['prompts'] = max(dev['prompts'], np.abs(_cplx(rec[h], a) - _cplx(ref[h], a)).max() / scale)
        for a in ('abs_e', 'abs_l'):
            dev['prompts'] = max(dev['prompts'], np.abs(rec[h][a] - ref[h][a]).max() / scale)
    dev['f_hz'] = np.abs(rec['f_hz'] - ref['f_hz']).max()
    dev['tau'] = np.abs(rec['tau'] - ref['tau']).max()
    both = ~np.isnan(ref['cn0_dbhz'])
    assert np.array_equal(np.isnan(rec['cn0_dbhz']), ~both)
    dev['cn0'] = np.abs(rec['cn0_dbhz'][both] - ref['cn0_dbhz'][both]).max()
    return dev


def check_numbers(dev, cs, what):
    print('deviations %s cs %d: ' % (what, cs) + '  '.join('%s %.3e' % kv for kv in dev.items()))
    for k, v in dev.items():
        assert v <= TOL[cs][k], (k, v, TOL[cs][k])


def check_decisions(rec, st, ref, rst, rnk, cs):
    """bit counts, every window start, and the hard bits where the restatement's are clear."""
    assert st['bit_no'].tolist() == [s['bit_no'] for s in rst]
    assert np.array_equal(rec['bit_no'], ref['bit_no'])
    for h in range(len(rec)):
        for b in range(rst[h]['bit_no']):
            _, _, n = W.windows(rec[h, b]['tau'], rec[h, b]['f_hz'], cs)
            assert np.array_equal(n, rnk[h, b]), (h, b)
        clear = np.abs(ref[h]['p_i']) > 0.1 * np.abs(_cplx(ref[h], 'p')).mean()
        assert np.array_equal(rec[h]['p_i'][clear] >= 0, ref[h]['p_i'][clear] >= 0)
        assert clear.sum() > len(clear) // 2
    got = np.array([int(t) for t in st['theta']], dtype=np.uint64)
    assert np.array_equal(st['prn'], [s['prn'] for s in rst])
    # (theta follows from the integer window starts and the increments: equal where f_hz agrees
    # to the bit, else close on the circle)
    for g, s in zip(got, rst):
        d = (int(g) - s['theta']) % (1 << 64)
        assert min(d, (1 << 64) - d) / 2.0 ** 64 < 1e-3


# ---- 1. decisions and numbers at 2048 -----------------------------------------------------------

@pytest.mark.parametrize('scene', ['weak', 'strong'])
def test_decisions_and_numbers(scene):
    amp = None if scene == 'weak' else W.STRONG_AMP
    sc, states, _ = W.opened(amp)
    ref, rst, rnk = W.tracked(amp)
    e = _engine(2048)
    try:
        rec, st = e.track_weak(W.scene_c64(amp), W.states_array(states), W.N_BITS)
        assert e.last_ms() > 0
    finally:
        e.close()
    check_decisions(rec, st, ref, rst, rnk, 2048)
    check_numbers(deviations(rec, ref), 2048, scene)
    check_truth(sc, rec[:5], [s['prn'] for s in states[:5]], strong=scene == 'strong')
    assert np.abs(rec[5]['lock']).max() < 0.5


# ---- 2. the same bytes from every input ---------------------------------------------------------

def test_same_bytes_from_every_input():
    """complex64 and raw u8, host and device input; one channel alone and among six, in any order;
    two calls; 45 bits in one call and 20 + 25 with the states carried over, the second chunk a
    slice with its own first_sample."""
    _, states, _ = W.opened()
    s0 = W.states_array(states)
    c64, raw = W.scene_c64(), np.ascontiguousarray(W.scene_raw())
    e, er = _engine(2048), _engine(2048, raw_u8=True)
    bufs = []
    try:
        rec, st = e.track_weak(c64, s0, W.N_BITS)
        for a, b in zip((rec, st), e.track_weak(c64, s0, W.N_BITS)):
            _same(a, b)
        for a, b in zip((rec, st), er.track_weak(raw, s0, W.N_BITS)):
            _same(a, b)
        for eng, arr in ((e, c64), (er, raw)):
            bufs.append(_upload(arr))
            for a, b in zip((rec, st), eng.track_weak((bufs[-1].ptr, len(arr)), s0, W.N_BITS)):
                _same(a, b)
        for h in (0, 3, 5):
            one, s1 = e.track_weak(c64, s0[h:h + 1], W.N_BITS)
            _same(one, rec[h:h + 1])
            _same(s1, st[h:h + 1])
        rev, srev = e.track_weak(c64, s0[::-1], W.N_BITS)
        _same(rev[::-1], rec)
        _same(srev[::-1], st)
        a, sa = e.track_weak(c64, s0, 20)
        first = int(np.floor(sa['tau']).min()) - 1
        b, sb = e.track_weak(c64[first:], sa, 25, first_sample=first)
        _same(np.concatenate([a, b], axis=1), rec)
        _same(sb, st)
        # ... and the raw slice on the device
        b2, sb2 = er.track_weak((bufs[1].at(2 * first), len(raw) - first), sa, 25, first_sample=first)
        _same(b2, b)
        _same(sb2, st)
    finally:
        for b in bufs:
            b.free()
        e.close()
        er.close()


# ---- 3. 16368 / taps at 8 samples -----------------------------------------------------------------

def test_hirate_12_bits():
    cs = 16368
    _, states, _ = W.opened(None, cs)
    ref, rst, rnk = W.tracked(None, cs)
    e = _engine(cs)
    try:
        rec, st = e.track_weak(W.scene_c64(None, cs), W.states_array(states), W.HIRATE_BITS, tap_samples=8)
        dflt = e.track_weak(W.scene_c64(None, cs), W.states_array(states), W.HIRATE_BITS)
    finally:
        e.close()
    _same(dflt[0], rec)                                   # 8 is the default at 16368
    check_decisions(rec, st, ref, rst, rnk, cs)
    check_numbers(deviations(rec, ref), cs, '12 bits')


# ---- 4. data that ends mid-span ---------------------------------------------------------------------

def test_short_data_stops_a_channel_and_no_other():
    """The code starts lie 412 .. 1650 samples into the data: with the data cut 600 samples behind
    the end of the first channel's 30th bit, the channels that start later than that fit 29 bits
    and the others 30 (the restatement on the cut data says which)."""
    from gpsmi._lib import WTRK_DATA_END
    _, states, _ = W.opened()
    s0 = W.states_array(states)
    c64 = W.scene_c64()
    e = _engine(2048)
    try:
        full, sf = e.track_weak(c64, s0, 30)
        ends = [int(np.floor(full[h, 29]['tau'])) + 20 * 2048 + 8 for h in range(6)]
        cut = ends[0] + 600
        short = [h for h in range(6) if ends[h] > cut]
        assert 0 < len(short) < 6
        rec, st = e.track_weak(c64[:cut], s0, 30)
        ref, rst, _ = W.track_ref(c64[:cut], states, 30, 2048)
    finally:
        e.close()
    print(ends, cut, st['bit_no'], st['flags'])
    assert st['bit_no'].tolist() == [s['bit_no'] for s in rst]
    for h in range(6):
        if h in short:
            assert st['bit_no'][h] == 29 and st['flags'][h] == WTRK_DATA_END
            _same(rec[h, :29], full[h, :29])
            assert not rec[h, 29:].view(np.uint8).any()
        else:
            assert st['bit_no'][h] == 30 and st['flags'][h] == 0
            _same(rec[h], full[h])
            _same(st[h:h + 1], sf[h:h + 1])


# ---- 5. command line ----------------------------------------------------------------------------------

def test_run_file_track(tmp_path):
    from conftest import ROOT
    path = tmp_path / 'deep.bin'
    np.ascontiguousarray(W.scene_raw()).tofile(path)
    base = [sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), str(path), '--seconds', '0.3',
            '--deep-acq', '1']
    r = subprocess.run(base + ['--refine', '--track', '--json'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])['deep_acquisition']
    truth = {p: f for p, f, _ in DEEP_HIGH + [DEEP_ZERO]}
    t = d['tracked']
    print(t)
    assert sorted(q['prn'] for q in t['channels']) == sorted(truth) and t['device_ms'] > 0
    for q in t['channels']:
        assert q['bits'] >= 45 and abs(q['f_hz'] - truth[q['prn']]) <= F_RMS_BOUND
        assert 22.0 <= q['cn0_dbhz'] <= 26.0 and 0 <= q['code_phase'] < 2048 and -1 <= q['lock'] <= 1
    r = subprocess.run(base + ['--track'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and '--track needs --refine' in r.stderr


# ---- what is refused --------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_usable():
    from gpsmi.engine import AcqEngine, Config, EngineError
    _, states, _ = W.opened()
    s0 = W.states_array(states)[:2]
    c64 = W.scene_c64()[:300 * 2048]
    e = _engine(2048)
    try:
        ok = e.track_weak(c64, s0, 5)
        for kw in (dict(n_bits=0), dict(n_bits=5, carrier_hz=float('nan')), dict(n_bits=5, first_sample=5000),
                   dict(n_bits=5, dll_bw=-1.0)):
            with pytest.raises(EngineError, match=r'\(-1\)'):
                e.track_weak(c64, s0, **kw)
        for a, b in zip(e.track_weak(c64, s0, 5), ok):
            _same(a, b)
    finally:
        e.close()
    e = AcqEngine(Config(code_samples=4096, n_cyc=8))
    try:
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.track_weak(np.zeros(50 * 4096, np.complex64), s0, 2)
    finally:
        e.close()
