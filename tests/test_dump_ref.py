"""Ties tests/dump_ref.py -- the float64 restatement of the prompt correlate-and-dump that
test_gpu_trk_dumps.py holds the correlators against -- to the frozen outputs of the reference
(tests/golden/ref_*.npz) and to the project's float32 oracle, and checks the condition on the
inputs that makes that comparison see a window boundary one sample off.  CPU only."""
import numpy as np
import pytest

import dump_ref as dr
import dump_scene as ds
from conftest import load_golden, scene_blocks
from test_oracle import CFG, ncyc_blocks

ORACLE_DUMP_TOL = 1e-4                # of the rms of the samples
SAMPLE_FLOOR = 0.49                   # smallest component of a sample of the boundary scene


def _config_id(cfg):
    return f'cs{cfg[0]}-ncyc{cfg[1]}'


@pytest.mark.parametrize('name', ['default', 'hirate', 'ncyc16', 'ncyc8'])
def test_dump_ref_equals_the_reference_fixture(name):
    """Every channel of a fixture chained over all its blocks: FREQ, PHASE and NPS at the start of
    block i are the fixture's values after block i - 1 (block 0: the opening state, FREQ still a
    Python float), DELAY is the fixture's for block i, and the carry is the tail sum dump_ref
    itself left behind block i - 1.  trk_dumps at the fixture tolerance, trk_n_dumps and trk_nps
    exactly."""
    g = load_golden(f'ref_{name}.npz')
    cs, n_cyc = CFG[name]['code_samples'], CFG[name]['n_cyc']
    nch, nb = g['trk_delay'].shape
    assert not g['trk_sweep'].any()                        # every block of the fixture was tracked
    blocks = scene_blocks(name, 5, nb) if name in ('default', 'hirate') else ncyc_blocks(name, 5, nb)
    worst = 0.0
    for c in range(nch):
        sv, f0, _ = g['trk_init'][c]
        st = dict(prn=int(sv), freq=np.float32(f0), omega0=np.float32(2 * np.pi * float(f0)),
                  phase=np.float32(0), nps=0, prev_sum_re=0.0, prev_sum_im=0.0)
        for i in range(nb):
            r = dr.dump_ref(blocks[i], st, int(g['trk_delay'][c, i]), cs, n_cyc)
            where = f'{name} channel {c} block {i}'
            nd = int(r['n_dumps'])
            assert nd == int(g['trk_n_dumps'][c, i]), where
            assert int(r['nps']) == int(g['trk_nps'][c, i]), where
            np.testing.assert_allclose(g['trk_dumps'][c, i, :nd], r['dumps'][:nd], rtol=1e-3, atol=1e-5,
                                       err_msg=where)
            worst = max(worst, float(np.max(np.abs(g['trk_dumps'][c, i, :nd] - r['dumps'][:nd])) / r['rms']))
            f = float(g['trk_freq'][c, i])
            assert np.float32(f) == f and np.float32(g['trk_phase'][c, i]) == g['trk_phase'][c, i], where
            clamped = abs(f) == 5000.0                     # confine() hands a Python float back
            st = dict(prn=int(sv), freq=np.float32(f), phase=np.float32(g['trk_phase'][c, i]),
                      omega0=np.float32(2 * np.pi * f) if clamped else np.float32(0),
                      nps=int(r['nps']), prev_sum_re=r['carry'].real, prev_sum_im=r['carry'].imag)
    print(f'{name}: reference fixture vs float64, worst |dump - ref| / rms {worst:.2e}')


_KINDS = ('edge', 'carry', 'signal')


def _table(kind, cs, n_cyc):
    """(blocks, table, forced) of one of the job tables of test_gpu_trk_dumps.py."""
    if kind == 'signal':
        return (ds.signal_blocks(cs, n_cyc)[0],) + ds.signal_table(cs, n_cyc)[:2]
    tab = ds.edge_table(cs, n_cyc) if kind == 'edge' else ds.carry_table(cs, n_cyc)
    return (ds.boundary_blocks(cs, n_cyc)[0],) + tab


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=_config_id)
def test_dump_ref_equals_the_oracle(cfg):
    """The job tables of test_gpu_trk_dumps.py through oracle_record (float32 carrier argument,
    complex64 wipe-off): n_dumps, first_len and the next nps equal on every job, every dump within
    1e-4 of the samples' rms."""
    cs, n_cyc = cfg
    for kind in _KINDS:
        blocks, table, forced = _table(kind, cs, n_cyc)
        ref, orc = ds.references(blocks, table, forced, cs, n_cyc, kind)
        ref, orc = ds.live(ref), ds.live(orc)
        _, worst = ds.bounds(orc, ref)
        print(f'CS {cs} N_CYC {n_cyc} {kind} table, {ref.size} jobs, oracle vs float64:',
              ' '.join(f'{k} {v:.2e}' for k, v in worst.items()),
              f'dump0 {dr.deviations(orc, ref)["dump0"].max():.2e} | rms {ref["rms"].mean():.3f}')
        assert worst['dumps'] <= ORACLE_DUMP_TOL, (kind, worst)
        assert set(ref['n_dumps']) == {n_cyc, n_cyc + 1} or kind == 'signal'
        if kind == 'signal':                                # the dumps carry signal, not only noise
            offs = ds.live(ds.signal_table(cs, n_cyc)[2])
            strong = (offs == 0) & (np.abs(ds.live(table['freq'])) == 5000.0)      # amplitude 0.12
            mag = np.abs(ref['dumps'][strong, 1:n_cyc])
            assert strong.sum() >= 2 and np.median(mag) > 0.06, np.median(mag)


def _boundary_changes(cs, n_cyc):
    """Over every job of the edge table, every boundary between two dumps and both directions: the
    smallest change that moving the boundary by one sample makes to either adjacent dump, and the
    number of (job, boundary, direction) cases.  A first boundary at the very start of the block
    (d = 0 behind a carry) cannot move to the left: the sample there belongs to the block before."""
    blocks, table, forced = _table('edge', cs, n_cyc)
    ref, _ = ds.references(blocks, table, forced, cs, n_cyc, 'edge')
    smallest, cases = np.inf, 0
    for i in range(table.shape[0]):
        for c in ds.LIVE:
            args = (blocks[i % ds.NB], table[i, c], int(forced[i, c]), cs, n_cyc)
            pre = dr.prefix(*args)
            ends = dr.window_ends(table[i, c]['nps'], forced[i, c], cs, n_cyc)
            for b in range(len(ends) - 1):
                for by in (-1, 1):
                    if ends[b] - int(table[i, c]['nps']) + by < 0:
                        continue
                    s = dr.shifted(*args, b, by, pre=pre)
                    change = np.abs(s['dumps'][b:b + 2] - ref[i, c]['dumps'][b:b + 2])
                    other = np.delete(np.abs(s['dumps'] - ref[i, c]['dumps']), [b, b + 1])
                    assert other.max() == 0
                    smallest = min(smallest, float(change.min()))
                    cases += 1
    return smallest, cases


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=_config_id)
def test_edge_table_sees_a_boundary_one_sample_off(cfg):
    """A condition on the inputs, checked with the references alone.  On the boundary-sensitive
    scene every component of a sample is at least 0.49 and the replica is +-1 on both sides of its
    own start, so (a) moving any boundary between two dumps of any job of the edge table by one
    sample changes both adjacent dumps by at least 0.49 / CS (the first windows of the table have at
    most CS + 3 samples: 0.49 sqrt(2) / (CS + 3) is above it); (b) the bound the GPU test puts on
    the dumps of these jobs -- 4 x the oracle's worst deviation from float64 -- is at most a quarter
    of that change, so (c) records with one boundary one sample off fail the GPU test's comparison
    by at least 4 x its bound."""
    cs, n_cyc = cfg
    blocks, table, forced = _table('edge', cs, n_cyc)
    ref, orc = ds.references(blocks, table, forced, cs, n_cyc, 'edge')
    assert int(ds.live(ref)['first_len'].max()) <= cs + 3
    bnds, worst = ds.bounds(ds.live(orc), ds.live(ref))
    smallest, cases = _boundary_changes(cs, n_cyc)
    rms = float(ds.live(ref)['rms'].max())
    print(f'CS {cs} N_CYC {n_cyc}: {cases} moved boundaries, smallest change of a dump {smallest:.3e} '
          f'(0.49 / CS = {SAMPLE_FLOOR / cs:.3e}); bound on the dumps {bnds["dumps"] * rms:.3e} '
          f'= {bnds["dumps"]:.2e} x rms {rms:.3f}')
    assert cases >= 2 * (n_cyc - 2) * ds.live(ref).size
    assert smallest >= SAMPLE_FLOOR / cs
    assert bnds['dumps'] * rms <= smallest / 4
    # (c) on one job per edge: the comparison of the GPU test, given such records
    for i in range(table.shape[0]):
        c = ds.LIVE[i % len(ds.LIVE)]
        args = (blocks[i % ds.NB], table[i, c], int(forced[i, c]), cs, n_cyc)
        b = (3 * i) % (int(ref[i, c]['n_dumps']) - 1)
        bad = ref.copy()
        bad[i, c] = dr.shifted(*args, b, 1)
        with pytest.raises(AssertionError) as err:
            ds.against_float64(ds.live(bad), ds.live(ref), bnds, 'one boundary moved')
        assert err.value.args[0][1] == 'dumps' and err.value.args[0][-1] >= 4, err.value.args[0]


def test_window_rules():
    """decodeData's window rules on hand-made states (gpslib.py:1408-1419, :1440)."""
    cs, n = 2048, 8
    assert dr.window_ends(0, 0, cs, n) == [cs * (i + 1) for i in range(n)]
    assert dr.window_ends(1, 0, cs, n) == [1 + cs * i for i in range(n + 1)]            # N_CYC + 1 dumps
    assert dr.window_ends(cs, 0, cs, n) == [cs * (i + 1) for i in range(n + 1)]
    assert dr.window_ends(2000, 100, cs, n) == [2100 + cs * i for i in range(n)]        # nps + d > CS
    assert dr.window_ends(0, 2047, cs, n) == [2047 + cs * i for i in range(n)]
    x = np.full(n * cs, 0.5 + 0.25j, np.complex64)
    st = dict(prn=9, freq=np.float32(0), omega0=np.float32(0), phase=np.float32(0), nps=cs,
              prev_sum_re=np.float32(3.0), prev_sum_im=np.float32(-1.0))
    r = dr.dump_ref(x, st, 0, cs, n)
    assert (r['n_dumps'], r['first_len'], r['nps'], r['carry']) == (n + 1, cs, 0, 0)
    assert r['dumps'][0] == (3.0 - 1.0j) / cs                # the carry alone
    rep = dr.replica(9, cs)
    np.testing.assert_allclose(r['dumps'][1:n + 1], np.mean(rep) * (0.5 + 0.25j), rtol=1e-12)
    st['nps'] = 0                                            # no carry: prev_sum belongs to no sample
    r = dr.dump_ref(x, st, 0, cs, n)
    assert (r['n_dumps'], r['first_len'], r['nps']) == (n, cs, 0)
    np.testing.assert_allclose(r['dumps'][0], np.mean(rep) * (0.5 + 0.25j), rtol=1e-12)
    st['nps'] = 3
    r = dr.dump_ref(x, st, 2047, cs, n)                      # 2050 samples in the first window
    assert (r['n_dumps'], r['first_len'], r['nps']) == (n, 2050, 1)
    want = ((3.0 - 1.0j) + np.sum(np.roll(rep, 2047)[:2047]) * (0.5 + 0.25j)) / 2050
    np.testing.assert_allclose(r['dumps'][0], want, rtol=1e-12)
    np.testing.assert_allclose(r['carry'], np.roll(rep, 2047)[2047] * (0.5 + 0.25j), rtol=1e-12)
    o = dr.oracle_record(x, st, 2047, cs, n)
    assert (o['n_dumps'], o['first_len'], o['nps']) == (n, 2050, 1)
    np.testing.assert_allclose(o['dumps'], r['dumps'], atol=1e-6)
