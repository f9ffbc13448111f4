"""The CPU side of the epilogue tests: tests/epilogue_ref.py is anchored to the real reference (the
four tracking fixtures, chained from their own dumps on its own state), the tables of
tests/epilogue_scene.py reach every listed case and keep the float32 oracle within the 1 % cap, and
every fault of FAULTS, applied to a copy of the reference, moves a job of every config."""
import numpy as np
import pytest

import dump_ref as dr
import dump_scene as ds
import epilogue_ref as er
import epilogue_scene as es
from conftest import load_golden

F32 = np.float32
CONFIG_IDS = [f'cs{cs}-ncyc{n}' for cs, n in ds.CONFIGS]
FIXTURES = {'ref_default': (2048, 32), 'ref_ncyc16': (2048, 16), 'ref_ncyc8': (2048, 8), 'ref_hirate': (16368, 8)}
FIRST_BLOCK = 5                      # the fixtures' tracking starts behind five acquisition blocks


def _ulps(a, b):
    return abs(float(a) - float(b)) / float(np.spacing(F32(max(abs(float(a)), abs(float(b)), 1e-30))))


@pytest.mark.parametrize('name', FIXTURES)
def test_reference_chained_over_the_fixture_reproduces_it(name):
    """epilogue_ref from the fixture's own dumps, on its own state (the oracle layer's float32 df
    and phase_shift feed the exact layer): lock flag, MS_TIME, len(EDGES) and the dump count exactly;
    FREQ, PHASE (mod 2 pi), STD_DEV and AMPLITUDE to float32 rounding (4 ulp; PHASE: of 2 pi)."""
    from gpsmi.engine import STATE_DTYPE
    cs, n_cyc = FIXTURES[name]
    g = load_golden(name + '.npz')
    cfg, ref = er.config(cs, n_cyc), er.Epilogue()
    assert not g['trk_sweep'].any()
    nch, nb = g['trk_delay'].shape
    for c in range(nch):
        st = np.zeros((), STATE_DTYPE)
        st['prn'], f0 = int(g['trk_init'][c, 0]), float(g['trk_init'][c, 1])
        st['freq'], st['omega0'] = F32(f0), F32(2 * np.pi * f0)
        st['df_len'], st['std_dev'] = 1, F32(0.005)
        ms_time, n_edges = 0, 1
        for i in range(nb):
            where = (name, 'channel', c, 'block', i)
            nd = int(g['trk_n_dumps'][c, i])
            dumps = g['trk_dumps'][c, i, :nd]
            o = er.tolerant_oracle(st, dumps, cfg)
            x = ref.exact(st, dumps, int(g['trk_delay'][c, i]), cfg, o['df'], o['phase_shift'])
            assert x['s_df_len'] == len(o['df_list']), where
            assert np.asarray(x['s_df'], F32).tobytes() == np.asarray(o['df_list'], F32).tobytes(), where
            ms_time += x['o_ms_count']
            n_edges += bin(x['o_edge_mask']).count('1')
            if st['phase_locked'] and (FIRST_BLOCK + i + 1) % cfg.df_no == 0 and n_edges > 2:
                n_edges = 2                                  # evalEdges keeps [sign, the last edge]
            assert o['locked'] == int(g['trk_locked'][c, i]), where
            assert ms_time == int(g['trk_ms_time'][c, i]), where
            assert n_edges == int(g['trk_n_edges'][c, i]), where
            assert x['o_n_dumps'] == nd
            assert _ulps(x['s_freq'], g['trk_freq'][c, i]) <= 4, where
            dph = (float(x['s_phase']) - g['trk_phase'][c, i] + np.pi) % (2 * np.pi) - np.pi
            assert abs(dph) <= 4 * np.spacing(F32(2 * np.pi)), where
            assert _ulps(o['std_dev'], g['trk_std_dev'][c, i]) <= 4, where
            assert _ulps(o['amplitude'], g['trk_amplitude'][c, i]) <= 4, where
            st['delay'] = x['s_delay']
            st['freq'], st['omega0'], st['phase'] = x['s_freq'], x['s_omega0'], x['s_phase']
            st['phase_locked'], st['std_dev'] = o['locked'], o['std_dev']
            st['edge_state'], st['prev_signal'] = x['s_edge_state'], x['s_prev_signal']
            st['df_len'] = x['s_df_len']
            st['df'][:x['s_df_len']] = x['s_df']


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=CONFIG_IDS)
def test_tables_reach_every_case_and_keep_the_oracle_within_the_cap(cfg):
    """With dump_ref's float64 dumps rounded to float32: nothing of coverage_gaps' list is missing,
    the bounds are positive, and the float32 oracle, judged like a kernel, leaves out at most 1 % of
    the live jobs.  The analytic rotation the table takes its dumps from equals dump_ref on the
    job's final state row."""
    cs, n_cyc = cfg
    jobs = es.cpu_jobs(cs, n_cyc)
    assert es.coverage_gaps(jobs, cs, n_cyc) == []
    c, ref = er.config(cs, n_cyc), er.Epilogue()
    r64 = [ref.tolerant64(st, g, c) for st, g, _ in jobs]
    orc = [er.tolerant_oracle(st, g, c) for st, g, _ in jobs]
    bounds, worst, left_out, bad = er.oracle_bounds(r64, orc)
    assert not bad, bad
    print(f'\nCS {cs} N_CYC {n_cyc}: oracle worst {worst}, left out {len(left_out)} of {len(jobs)}')
    assert len(left_out) <= len(jobs) // 100
    blks, _ = es.blocks(cs, n_cyc)
    tab, forced, dumps = es.table(cs, n_cyc)
    for i, ch in ((0, 0), (9, 3), (13, 12), (47, 7)):
        r = dr.dump_ref(blks[i % ds.NB], tab[i, ch], int(forced[i, ch]), cs, n_cyc)
        assert int(r['n_dumps']) == len(dumps[i, ch])
        assert np.abs(r['dumps'][:len(dumps[i, ch])] - dumps[i, ch]).max() < 1e-7 * np.abs(dumps[i, ch]).max()


# ---- one fault at a time, applied to a copy of the reference

class WrongNeighbour(er.Epilogue):
    """the neighbour of ONE dump (self.at: 8 / 16 / 24 / N_CYC) taken from the wrong element (a lane
    further) on ONE path (self.path: the edge scan's fetch or the unwrap's)"""
    at, path = None, None

    def before(self, re, i, prev_signal0):
        wrong = self.path == 'scan' and i == self.at
        return re[i - 2] if wrong else super().before(re, i, prev_signal0)

    def neighbour(self, ph, i):
        return ph[i - 2] if self.path == 'unwrap' and i == self.at else ph[i - 1]


class UnwrapSignSwapped(er.Epilogue):
    def unwrap_step(self, delta):
        return -super().unwrap_step(delta)


class UnwrapMissesLastDump(er.Epilogue):
    def unwrap_range(self, n):
        return range(1, n - 1)


class SumWithoutTail(er.Epilogue):
    """a sum that drops its tail elements when n % 8 != 0"""
    def total(self, a):
        return np.sum(a[:len(a) - len(a) % 8]) if len(a) >= 8 else np.sum(a)


class ShiftOffByOne(er.Epilogue):
    def shifted(self, lst):
        return lst[2:] + lst[-1:]


class FullReadAsGreater(er.Epilogue):
    def list_full(self, n, df_no):
        return n > df_no


class ClampSignLost(er.Epilogue):
    def clamp(self, df, max_df):
        return max_df


class ThresholdReadAsGreaterEqual(er.Epilogue):
    def step_large(self, step, thr):
        return step >= thr


class ZeroPrevSignalPositive(er.Epilogue):
    def carries_sign(self, p, prev):
        return prev >= 0 if p > 0 else prev < 0


class Bit32Dropped(er.Epilogue):
    def mask_word(self, mask):
        return mask & 0xFFFFFFFF


FAULTS = (UnwrapSignSwapped, UnwrapMissesLastDump, SumWithoutTail, ShiftOffByOne,
          FullReadAsGreater, ClampSignLost, ThresholdReadAsGreaterEqual, ZeroPrevSignalPositive, Bit32Dropped)


def _cpu_reference(cs, n_cyc):
    """(jobs, their float64 fields, the oracle's bounds) of a config's table, once."""
    def make():
        c, ref = er.config(cs, n_cyc), er.Epilogue()
        jobs = es.cpu_jobs(cs, n_cyc)
        r64 = [ref.tolerant64(st, g, c) for st, g, _ in jobs]
        bounds, _, _, bad = er.oracle_bounds(r64, [er.tolerant_oracle(st, g, c) for st, g, _ in jobs])
        assert not bad, bad
        return jobs, r64, bounds
    return ds.memo(('epilogue cpu reference', cs, n_cyc), make)


def _moved(cs, n_cyc, faulty):
    """Does a job of the table move an exact field, or a toleranced one by more than 4 x its bound?"""
    c, ref = er.config(cs, n_cyc), er.Epilogue()
    jobs, r64, bounds = _cpu_reference(cs, n_cyc)
    for (st, g, d), good in zip(jobs, r64):
        bad = faulty.tolerant64(st, g, c)
        if bad['locked'] != good['locked']:
            return True
        if any(abs(bad[k] - good[k]) / (abs(good[k]) if k in ('std_dev', 'amplitude') else 1.0) > 4 * bounds[k]
               for k in er.TOLERANCED):
            return True
        df, shift = F32(good['df']), F32(good['phase_shift'])
        a, b = ref.exact(st, g, d, c, df, shift), faulty.exact(st, g, d, c, df, shift)
        if any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() for k in a):
            return True
    return False


@pytest.mark.parametrize('fault', FAULTS, ids=[f.__name__ for f in FAULTS])
def test_every_fault_moves_a_job_of_every_config(fault):
    """Each fault the issue lists, on the tables: a job of every config moves.  Bit 32 of the edge
    mask exists at N_CYC = 32 alone (the other configs have at most 17 dumps): there the fault is
    shown at that config and is shown to change nothing at the others."""
    for cs, n_cyc in ds.CONFIGS:
        moved = _moved(cs, n_cyc, fault())
        if fault is Bit32Dropped and n_cyc < 32:
            assert not moved
        else:
            assert moved, (fault.__name__, cs, n_cyc)


@pytest.mark.parametrize('path', ['scan', 'unwrap'])
@pytest.mark.parametrize('at', [8, 16, 24, 'N_CYC'])
def test_a_wrong_neighbour_moves_a_job_of_every_config(at, path):
    """The neighbour of one dump -- 8, 16, 24 (the first of an eight-lane group) or N_CYC (the extra
    dump) -- fetched from a lane further, on one path alone (the edge scan's or the unwrap's): a job
    moves at every config that has that dump; where N_CYC is too short to have it, nothing does."""
    for cs, n_cyc in ds.CONFIGS:
        faulty = WrongNeighbour()
        faulty.at, faulty.path = (n_cyc if at == 'N_CYC' else at), path
        assert _moved(cs, n_cyc, faulty) == (faulty.at <= n_cyc), (at, path, cs, n_cyc)


def test_a_record_that_is_not_a_number_fails():
    """compare_job on records that are right in every field (built from the reference itself) passes;
    the same records with NaN in std_dev and amplitude, or in df and phase_shift -- the next state
    row consistent with the record, as a kernel writes it -- fail on every job: none passes, none is
    left out, and the deviation returned is NaN, so that the printed figure shows it."""
    from gpsmi.engine import OUT_DTYPE, STATE_DTYPE
    cs, n_cyc = 2048, 8
    c, ref = er.config(cs, n_cyc), er.Epilogue()
    jobs, r64, bounds = _cpu_reference(cs, n_cyc)
    checked = 0
    for (st, g, d), t in zip(jobs[:60], r64):
        for nan in ((), ('std_dev', 'amplitude'), ('df', 'phase_shift')):
            rec, nxt = np.zeros((), OUT_DTYPE), np.zeros((), STATE_DTYPE)
            for k in er.TOLERANCED:
                rec[k] = np.nan if k in nan else F32(t[k])
            rec['n_dumps'], rec['phase_locked'] = len(g), t['locked']
            rec['dumps'][0:2 * len(g):2], rec['dumps'][1:2 * len(g):2] = g.real, g.imag
            x = ref.exact(st, g, d, c, rec['df'], rec['phase_shift'])
            rec['edge_mask'], rec['edge_mask_hi'] = x['o_edge_mask'] & 0xFFFFFFFF, x['o_edge_mask'] >> 32
            for k in ('edge_sign0', 'ms_count', 'freq', 'phase'):
                rec[k] = x['o_' + k]
            for k in ('prn', 'delay', 'edge_state', 'prev_signal', 'freq', 'phase', 'omega0', 'df_len'):
                nxt[k] = x['s_' + k]
            nxt['df'][:x['s_df_len']] = x['s_df']
            nxt['std_dev'], nxt['phase_locked'], nxt['nps'] = rec['std_dev'], rec['phase_locked'], rec['nps']
            bad, dev, left_out, _ = er.compare_job(ref, st, rec, nxt, d, c, bounds)
            if not nan:
                assert not bad and (left_out or dev is not None), (bad, st)
                continue
            assert bad and not left_out, (nan, st)
            assert {b[0] for b in bad} >= set(nan), bad
            assert all(np.isnan(dev[k]) for k in nan)
            checked += 1
    assert checked == 120
