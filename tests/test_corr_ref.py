"""Ties tests/corr_ref.py -- the float64 restatement of the code-phase correlation that
test_gpu_trk_corr.py holds the kernel against -- to the project's float32 oracle and to the frozen
outputs of the reference (tests/golden/ref_default.npz).  CPU only."""
import numpy as np
import pytest

import corr_ref as cr
import gps_oracle as orc
from conftest import scene_blocks

# (N_CYC, CORR_AVG): the reference's pair, a short block folded whole (first = 0), the unpiped fold
PAIRS = ((32, 8), (8, 8), (16, 5))
ABSENT = (1, 33, 34, 37)              # default_scene draws from 2 .. 32

REL_FIELDS = ('epl', 'corr_mean', 'corr_std', 'norm_max_corr')
# Worst relative deviation of the oracle from corr_ref allowed per field: some twice the largest
# figure the two tests below measured (their docstrings).  The oracle's carrier phase
# argument is float32: phase + om t reaches 1000 rad at the end of a 32-ms block, where a float32
# ulp is 6e-5 rad, so a coherent sum over 8 periods is off by some 1e-5 of its magnitude at most.
ORACLE_RTOL = {'epl': 4e-5, 'corr_mean': 3e-6, 'corr_std': 4e-6, 'norm_max_corr': 3e-5}
ORACLE_CP_ATOL = 1e-5                 # samples


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))


def _states_of(sc, block_no, rng):
    """One state row per satellite of the scene and per absent PRN.  Block 0: FREQ is a Python
    float on a 10-Hz grid (omega0 set) and PHASE 0, as after initInst; later blocks: FREQ a
    float32 off the grid (omega0 = 0) and PHASE anywhere in [0, 2 pi)."""
    rows = []
    prns = [s.prn for s in sc.sats] + list(ABSENT)
    for i, prn in enumerate(prns):
        dop = sc.sats[i].doppler if i < len(sc.sats) else -4000.0 + 2400.0 * (i - len(sc.sats))
        f0 = round(dop / 10.0) * 10.0
        if block_no == 0:
            st = dict(prn=prn, freq=np.float32(f0), omega0=np.float32(2 * np.pi * f0),
                      phase=np.float32(0), delay=0)
        else:
            st = dict(prn=prn, freq=np.float32(dop + rng.uniform(-20, 20)), omega0=np.float32(0),
                      phase=np.float32(rng.uniform(0, 2 * np.pi)), delay=int(rng.integers(0, 2048)))
        rows.append(st)
    return rows


@pytest.mark.parametrize('n_cyc,corr_avg', PAIRS)
def test_corr_ref_equals_the_oracle(n_cyc, corr_avg):
    """corr_ref against SatStream.cacode_corr (float32 carrier phase, complex64 wipe-off and
    forward FFT) on default_scene(12, seed=5, amp=0.09) plus four absent PRNs, blocks 0 .. 2:
    same argmax and CORR_MIN decision for every job, the real-valued fields within ORACLE_RTOL.
    Measured worst relative deviations (N_CYC, CORR_AVG), 48 jobs each:
                   epl      corr_mean  corr_std  norm_max_corr  code_phase (samples)
        (32, 8)   8.4e-6    8.2e-7     1.1e-6    5.7e-6         8.0e-7
        (8, 8)    1.7e-6    2.7e-7     3.7e-7    1.6e-6         3.4e-7
        (16, 5)   3.8e-6    5.0e-7     5.7e-7    5.3e-6         1.2e-6
    Both sides of CORR_MIN occur; the smallest gap between the two largest lags is 3.4e-3 of the
    peak: no argmax here is a matter of rounding."""
    from gpsmi import synth
    sc = synth.default_scene(12, seed=5, n_cyc=n_cyc, amp=0.09)
    assert not set(ABSENT) & {s.prn for s in sc.sats}
    rng = np.random.default_rng(100 * n_cyc + corr_avg)
    worst = dict.fromkeys(REL_FIELDS + ('code_phase',), 0.0)
    found, gap_present, gap_all = [], 1.0, 1.0
    for b in range(3):
        blk = sc.block(b)
        for st in _states_of(sc, b, rng):
            r = cr.corr_ref(blk, st, n_cyc, corr_avg, 8.0)
            o = cr.oracle_record(blk, st, n_cyc, corr_avg, 8.0)
            where = f'block {b} prn {st["prn"]}'
            assert r['mx'] == o['mx'], where
            assert r['delay'] == o['delay'] and r['delay_used'] == o['delay_used'], where
            for k in REL_FIELDS:
                worst[k] = max(worst[k], _rel(o[k], r[k]))
            if r['delay'] >= 0:
                worst['code_phase'] = max(worst['code_phase'], abs(float(o['code_phase'] - r['code_phase'])))
            else:
                assert r['code_phase'] == -1.0 and r['delay_used'] == st['delay']
            found.append(bool(r['delay'] >= 0))
            gap_all = min(gap_all, float(r['gap']))
            if st['prn'] not in ABSENT:
                gap_present = min(gap_present, float(r['gap']))
    print(f'(N_CYC {n_cyc}, CORR_AVG {corr_avg}) oracle vs float64:',
          ' '.join(f'{k} {v:.2e}' for k, v in worst.items()),
          f'| smallest top-two gap {gap_all:.2e}, of a present PRN {gap_present:.2e}')
    assert any(found) and not all(found)
    assert gap_all > 1e-4
    for k in REL_FIELDS:
        assert worst[k] <= ORACLE_RTOL[k], (k, worst[k])
    assert worst['code_phase'] <= ORACLE_CP_ATOL


def test_corr_ref_equals_the_reference_fixture(golden_default):
    """The fixture's own trajectory: the oracle streams replayed forward over blocks 5 .. 52 of the
    default scene give the state at the start of every block (FREQ a Python float until the loop
    makes it a float32); corr_ref on those states against the reference's recorded trk_mx,
    trk_epl, trk_corr_mean, trk_corr_std, trk_norm, trk_delay and trk_code_phase.  Measured worst
    deviations over the 576 jobs: epl 1.6e-5, corr_mean 1.1e-6, corr_std 1.7e-6, norm 1.2e-5
    (relative), code_phase 3.2e-6 samples."""
    g = golden_default
    p = orc.Params()
    nch, nb = g['trk_delay'].shape
    blocks = scene_blocks('default', 5, nb)
    worst = dict.fromkeys(REL_FIELDS + ('code_phase',), 0.0)
    for c in range(nch):
        sv, f0, d0 = g['trk_init'][c]
        ss = orc.SatStream(int(sv), float(f0), p, delay=int(d0))
        for i in range(nb):
            py_float = not isinstance(ss.freq, np.floating)
            st = dict(prn=int(sv), freq=np.float32(ss.freq), phase=np.float32(ss.phase), delay=int(ss.delay),
                      omega0=np.float32(2 * np.pi * float(ss.freq)) if py_float else np.float32(0))
            assert float(st['phase']) == float(ss.phase)          # the state is float32 already
            r = cr.corr_ref(blocks[i], st, p.n_cyc, p.corr_avg, p.corr_min)
            ss.process(blocks[i], np.int64((5 + i + 1) * p.ngps))
            where = f'channel {c} block {i}'
            assert r['mx'] == g['trk_mx'][c, i], where
            found = r['delay'] >= 0
            assert found == (g['trk_code_phase'][c, i] >= 0), where
            assert r['delay_used'] == g['trk_delay'][c, i], where
            got = dict(epl=g['trk_epl'][c, i], corr_mean=g['trk_corr_mean'][c, i],
                       corr_std=g['trk_corr_std'][c, i], norm_max_corr=g['trk_norm'][c, i])
            for k in REL_FIELDS:
                worst[k] = max(worst[k], _rel(got[k], r[k]))
            if found:
                worst['code_phase'] = max(worst['code_phase'],
                                          abs(float(g['trk_code_phase'][c, i] - r['code_phase'])))
    print('reference fixture vs float64:', ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    for k in REL_FIELDS:
        assert worst[k] <= ORACLE_RTOL[k], (k, worst[k])
    assert worst['code_phase'] <= ORACLE_CP_ATOL


def test_decode_and_record_rules():
    """The unpack formula against the generator's own decode, and corr_finish's choice of DELAY
    on a surface built by hand."""
    from gpsmi import synth
    raw = np.arange(65536, dtype=np.uint16)                # every (I, Q) byte pair
    assert cr.decode_u8(raw).tobytes() == synth.raw_to_c64(raw).tobytes()
    corr = np.full(2048, 1.0)
    corr[::2] = 1.2
    corr[0], corr[2047], corr[1] = 30.0, 12.0, 9.0         # peak at lag 0: neighbours wrap
    r = cr.corr_record(corr, 8.0, 77, -1)
    assert (r['mx'], r['delay'], r['delay_used']) == (0, 0, 0)
    assert tuple(r['epl']) == (12.0, 30.0, 9.0)
    assert r['code_phase'] == orc.fit_code_phase(corr, 0) < 0
    assert cr.corr_record(corr, 8.0, 77, 5)['delay_used'] == 5
    weak = cr.corr_record(corr, 1e9, 77, -1)               # below CORR_MIN: the state's delay
    assert (weak['delay'], weak['code_phase'], weak['delay_used']) == (-1, -1.0, 77)
    assert cr.corr_record(corr, 1e9, 77, 0)['delay_used'] == 0
    assert r['gap'] == pytest.approx(18.0 / 30.0)
    assert cr.omega_f32(1000.0, 0.0) == np.float32(2 * np.pi) * np.float32(1000.0)
    assert cr.omega_f32(1000.0, np.float32(5.5)) == np.float32(5.5)
