"""The tracking epilogue -- trk_epilogue_span_kernel<NC>, trk_epilogue8_kernel<NC>,
trk_epilogue_kernel, trk_epilogue_span8_kernel and the batch epilogues behind the vector correlator
-- against its CPU restatement (tests/epilogue_ref.py), every form the handle reports running, on
the tables of tests/epilogue_scene.py: rows the closed loop does not visit.

Every job starts from the kernel's own prompt dumps (the windows behind them are pinned by
test_gpu_trk_dumps.py).  Exact layer (edge scan, carrier, drift list, copied words): bitwise on
every live job.  Toleranced layer (std_dev, amplitude, phase_shift, df): the deviation from float64
within 4 x the float32 oracle's own worst deviation from float64 over the same jobs, the bounds
computed here from the form's dumps; a job next to a decision threshold whose decision differs
from float64's is left out, at most 1 % of the live jobs.  The coverage list of
epilogue_scene.coverage_gaps is asserted on every form's own dumps.  A toleranced field that is NaN
fails, and shows as NaN in the printed figures.  The test prints the table DESIGN.md section 4.5 is to
carry: the oracle's figure and every form's, per config."""
import numpy as np
import pytest

import dump_scene as ds
import epilogue_ref as er
import epilogue_scene as es

pytestmark = pytest.mark.gpu

CONFIG_IDS = [f'cs{cs}-ncyc{n}' for cs, n in ds.CONFIGS]
# (family, form, epilogue_form or None where the handle has no choice)
FORMS = {2048: (('span', 'single', None), ('span', 'batch', 1), ('span', 'batch', 0),
                ('vector', 'one launch', 1), ('vector', 'one launch', 0)),
         16368: (('span8', 'ranges', None), ('vector', 'chunked', 1), ('vector', 'chunked', 0)),
         4096: (('vector', 'chunked', 1), ('vector', 'chunked', 0))}


_RUNS = {}


def _run(cs, n_cyc):
    """{form: (records, next states)} of the table through every form, once."""
    if (cs, n_cyc) not in _RUNS:
        _RUNS[cs, n_cyc] = _run_forms(cs, n_cyc)
    return _RUNS[cs, n_cyc]


def _run_forms(cs, n_cyc):
    from gpsmi.engine import DeviceBuffer
    blks, _ = es.blocks(cs, n_cyc)
    table, forced, _ = es.table(cs, n_cyc)
    prns = sorted(set(int(p) for p in table['prn'].ravel()) - {0})
    units = ds.NB * ((ds.NCH + 11) // 12)
    buf = DeviceBuffer(len(blks) * blks[0].nbytes)
    engines, got = {}, {}
    try:
        buf.upload(np.stack(blks))
        for family, form, epi in FORMS[cs]:
            if family not in engines:
                engines[family] = ds.engine(cs, n_cyc, family, prns)
            eng = engines[family]
            if family == 'span':
                if form == 'batch':                          # (the single-block form: the default threshold)
                    eng.set_option('span_single_max', 1)
                assert (units <= eng.get_option('span_single_max')) == (form == 'single'), (form, units)
            if epi is not None:
                eng.set_option('epilogue_form', epi)
                assert eng.get_option('epilogue_form') == epi
            got[family, form, epi] = ds.replay(eng, buf, blks[0].nbytes, table, forced)
    finally:
        buf.free()
        for e in engines.values():
            e.close()
    return got


def _check_form(name, out, nxt, table, forced, cs, n_cyc):
    """One form against the reference; returns (failures, figures)."""
    ref, cfg = er.Epilogue(), er.config(cs, n_cyc)
    failures = []
    closed = list(ds.CLOSED)
    if out[:, closed].tobytes() != bytes(out[:, closed].nbytes):
        failures.append((name, 'closed channels: record not all-zero'))
    if nxt[:, closed].tobytes() != table[:, closed].tobytes():
        failures.append((name, 'closed channels: state row not copied through'))
    idx = [(i, c) for i in range(table.shape[0]) for c in ds.LIVE]
    if not np.array_equal(ds.live(out['delay_used']), ds.live(forced)):
        failures.append((name, 'delay_used'))
    jobs = [(table[i, c], er.job_dumps(out[i, c]), int(forced[i, c])) for i, c in idx]
    r64 = [ref.tolerant64(st, g, cfg) for st, g, _ in jobs]
    orc = [er.tolerant_oracle(st, g, cfg) for st, g, _ in jobs]
    bounds, worst_orc, orc_out, bad = er.oracle_bounds(r64, orc)
    failures += [(name,) + b for b in bad]
    worst = dict.fromkeys(er.TOLERANCED, 0.0)
    left_out = 0
    for (i, c), (st, _, d) in zip(idx, jobs):
        bad, dev, out_of_it, _ = er.compare_job(ref, st, out[i, c], nxt[i, c], d, cfg, bounds)
        for b in bad:
            failures.append((name, 'job', (i, c)) + b)
        left_out += out_of_it
        if dev is not None:
            for k in er.TOLERANCED:
                worst[k] = float(np.maximum(worst[k], dev[k]))        # (a NaN stays in the figure)
    if left_out > len(idx) // 100:
        failures.append((name, 'left out', left_out, 'of', len(idx)))
    if len(orc_out) > len(idx) // 100:
        failures.append((name, 'the oracle leaves out', len(orc_out), 'of', len(idx)))
    gaps = es.coverage_gaps(jobs, cs, n_cyc)
    if gaps:
        failures.append((name, 'not covered', gaps))
    return failures, (worst_orc, worst, left_out, len(orc_out))


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=CONFIG_IDS)
def test_epilogue_against_the_reference(cfg):
    """Every form of the epilogue at this config on the off-trajectory table: locked, unlocked and
    locking rows, an edge on every dump 0 .. N_CYC, every edge_state, PREV_SIGNAL of either sign and
    0, STD_DEV 0 and huge, unwrap steps of either sign on every dump, drift lists of every listed
    length with and without the shift, the df clamp and the FREQ clamp at either end."""
    cs, n_cyc = cfg
    table, forced, _ = es.table(cs, n_cyc)
    got = _run(cs, n_cyc)
    assert set(got) == set(FORMS[cs])
    print(f'\nepilogue table, CS {cs} N_CYC {n_cyc}: {table.shape[0] * len(ds.LIVE)} live jobs; '
          'worst deviation from float64 (std_dev, amplitude relative; phase_shift rad; df Hz)')
    print(f'    {"":<26} ' + ' '.join(f'{k:>11}' for k in er.TOLERANCED) + '  left out')
    failures = []
    for form, (out, nxt) in got.items():
        name = ' '.join(str(f) for f in form if f is not None)
        bad, (worst_orc, worst, left, orc_left) = _check_form(name, out, nxt, table, forced, cs, n_cyc)
        print(f'    {"oracle, on its dumps":<26} ' + ' '.join(f'{worst_orc[k]:>11.2e}' for k in er.TOLERANCED)
              + f'  {orc_left}')
        print(f'    {name:<26} ' + ' '.join(f'{worst[k]:>11.2e}' for k in er.TOLERANCED) + f'  {left}')
        failures += bad
    assert not failures, failures[:20]


@pytest.mark.parametrize('n_cyc', [32, 16, 8])
def test_batch_forms_are_bytewise_equal_on_the_table(n_cyc):
    """The two batch epilogues behind the span correlator write the same bytes on this table too
    (records whole, next states up to the drift list's length)."""
    got = _run(2048, n_cyc)
    (o1, n1), (o0, n0) = got['span', 'batch', 1], got['span', 'batch', 0]
    assert o1.tobytes() == o0.tobytes()
    for k in n1.dtype.names:
        if k != 'df':
            assert n1[k].tobytes() == n0[k].tobytes(), k
    for idx in np.ndindex(n1.shape):
        n = int(n1[idx]['df_len'])
        assert n1[idx]['df'][:n].tobytes() == n0[idx]['df'][:n].tobytes(), idx
