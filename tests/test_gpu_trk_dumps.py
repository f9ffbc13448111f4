"""The prompt correlate-and-dump -- trk_span_kernel<1, 1> and <8, 4> with complex64 and raw uint16
input at N_CYC = 32 / 16 / 8, trk_span8_kernel, trk_stream_kernel with and without
trk_partial_reduce_kernel -- against the float64 restatement of the operation (tests/dump_ref.py),
every form the handle reports running.

Everything goes through TrkEngine.replay with a state table and forced delays (delay_used is the
forced delay, asserted); replay_states supplies the next nps and prev_sum.  Per (block, channel)
job: n_dumps, first_len, the next nps and delay_used exactly, no job left out; the dumps and the
next prev_sum within 4 x the float32 oracle's own worst deviation from float64 over the same jobs
(the oracle carries a float32 carrier argument, the kernels a double-reduced one: a correct
kernel has room to spare; the factor covers the different but legitimate orders of the float32
sums).  The bounds are computed in the tests from those jobs; tests/test_dump_ref.py shows on the
CPU that on the edge table they lie at most at a quarter of what one sample on the wrong side of
a window boundary changes.  DESIGN.md section 4.4 has the figures of an MI355X run.

Launches are at most 16 blocks x 13 channels: two channel groups of the span correlators, the
second with one live column, channels 5 and 6 closed."""
import numpy as np
import pytest

import dump_ref as dr
import dump_scene as ds

pytestmark = pytest.mark.gpu

CONFIG_IDS = [f'cs{cs}-ncyc{n}' for cs, n in ds.CONFIGS]
# what runs at each code length: (family, form, input format); a family's forms are bytewise equal
FORMS = {2048: (('span', 'single', 'c64'), ('span', 'single', 'u8'), ('span', 'batch', 'c64'),
                ('span', 'batch', 'u8'), ('vector', 'one launch', 'c64')),
         16368: (('span8', 'ranges', 'c64'), ('vector', 'chunked', 'c64')),
         4096: (('vector', 'chunked', 'c64'),)}

_RUNS = {}


def _run(kind, cs, n_cyc):
    """{(family, form, format): (records, next states)} of a table through every form, once."""
    key = (kind, cs, n_cyc)
    if key in _RUNS:
        return _RUNS[key]
    from gpsmi.engine import DeviceBuffer
    c64, raws, table, forced = _scene_and_table(kind, cs, n_cyc)
    prns = sorted(set(int(p) for p in table['prn'].ravel()) - {0})
    units = min(ds.NB, table.shape[0]) * ((ds.NCH + 11) // 12)
    bufs, engines, got = {}, {}, {}
    try:
        for fmt, src in (('c64', c64), ('u8', raws)):
            if any(f[2] == fmt for f in FORMS[cs]):
                bufs[fmt] = DeviceBuffer(len(src) * src[0].nbytes)
                bufs[fmt].upload(np.stack(src))
        for family, form, fmt in FORMS[cs]:
            if family not in engines:
                engines[family] = ds.engine(cs, n_cyc, family, prns)
            eng = engines[family]
            if family == 'span':
                if form == 'batch':                          # (the single-block form: the default threshold)
                    eng.set_option('span_single_max', 1)
                single = units <= eng.get_option('span_single_max')
                assert single == (form == 'single'), (form, units)
                eng.set_input_format(fmt == 'u8')
            src = c64 if fmt == 'c64' else raws
            got[family, form, fmt] = ds.replay(eng, bufs[fmt], src[0].nbytes, table, forced)
    finally:
        for b in bufs.values():
            b.free()
        for e in engines.values():
            e.close()
    _RUNS[key] = got
    return got


def _scene_and_table(kind, cs, n_cyc):
    if kind == 'signal':
        c64, raws, _ = ds.signal_blocks(cs, n_cyc)
        table, forced, _ = ds.signal_table(cs, n_cyc)
    else:
        c64, raws = ds.boundary_blocks(cs, n_cyc)
        table, forced = ds.edge_table(cs, n_cyc) if kind == 'edge' else ds.carry_table(cs, n_cyc)
    return c64, raws, table, forced


def _check(kind, cs, n_cyc):
    """A table through every form, each against float64, with the figures printed.  Returns the
    float64 records of the live jobs."""
    c64, _, table, forced = _scene_and_table(kind, cs, n_cyc)
    ref, orc = ds.references(c64, table, forced, cs, n_cyc, kind)
    ref, orc = ds.live(ref), ds.live(orc)
    bnds, _ = ds.bounds(orc, ref)
    orc_dev = dr.deviations(orc, ref)
    got = _run(kind, cs, n_cyc)
    assert set(got) == set(FORMS[cs])
    print(f'\n{kind} table, CS {cs} N_CYC {n_cyc}: {ref.size} jobs; worst deviation from float64 / rms')
    print(f'    {"":<28} {"dumps":>10} {"dump0":>10} {"prev_sum":>10}')
    print(f'    {"oracle":<28} ' + ' '.join(f'{float(np.max(orc_dev[k])):>10.2e}' for k in dr.REPORTED))
    failures = []
    for form, (out, nxt) in got.items():
        closed = out[:, list(ds.CLOSED)]
        assert (closed['prn'] == 0).all() and (closed['n_dumps'] == 0).all(), form
        assert (out['prn'] == table['prn']).all(), form
        assert np.array_equal(ds.live(out['delay_used']), ds.live(forced)), (form, 'delay_used')
        assert np.array_equal(ds.live(nxt['nps']), ds.live(out['nps'])), (form, 'nps of the next state')
        recs = ds.live(dr.kernel_records(out, nxt))
        dev = dr.deviations(recs, ref)
        print(f'    {" ".join(form):<28} ' + ' '.join(f'{float(np.max(dev[k])):>10.2e}' for k in dr.REPORTED))
        try:
            ds.against_float64(recs, ref, bnds, (kind, cs, n_cyc) + form)
        except AssertionError as e:                          # every form is printed before one fails
            failures.append(e.args[0])
    assert not failures, failures
    return ref


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=CONFIG_IDS)
def test_edge_table_against_float64(cfg):
    """The window boundary on every place a correlator treats specially (dump_scene.EDGES: the
    list of test_forced_delays_at_every_edge_agree_across_correlators at CS = 2048, the tile /
    range / chunk / period edges of the other code lengths), every edge in every column of the 13
    channels, on the boundary-sensitive scene with its three carriers: FREQ -5000, +5000, 0 and two
    values between, with and without omega0, PHASE 0 and the largest float32 below 2 pi."""
    cs, n_cyc = cfg
    ref = _check('edge', cs, n_cyc)
    assert set(ref['n_dumps']) == {n_cyc, n_cyc + 1}


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=CONFIG_IDS)
def test_carry_table_against_float64(cfg):
    """The state kinds of random_state_runs (dump_scene.carry_table): no carry and delay 0; a carry
    and delay 0 (N_CYC + 1 dumps); nps + d > CS; nps = CS; a first window of a few samples; a drawn
    prev_sum throughout.  dump[0], n_dumps, first_len, the next nps and the next prev_sum."""
    cs, n_cyc = cfg
    ref = _check('carry', cs, n_cyc)
    assert set(ref['n_dumps']) == {n_cyc, n_cyc + 1}
    assert ref['first_len'].min() <= 6 and ref['first_len'].max() > cs


@pytest.mark.parametrize('cfg', ds.CONFIGS, ids=CONFIG_IDS)
def test_signal_scene_against_float64(cfg):
    """The satellites of test_gpu_trk_corr.py at their Doppler with the window boundary at the
    true code start and up to two samples off it: dumps that carry signal, not only noise."""
    cs, n_cyc = cfg
    ref = _check('signal', cs, n_cyc)
    assert np.abs(ref['dumps'][:, 1:n_cyc]).max() > 0.06


@pytest.mark.parametrize('n_cyc', [32, 16, 8])
def test_forms_of_the_span_correlator_are_bytewise_equal(n_cyc):
    """Within the span family the records and next states of all forms are the same bytes on these
    tables too: single-block == batch, raw uint16 == complex64."""
    for kind in ('edge', 'carry', 'signal'):
        got = _run(kind, 2048, n_cyc)
        span = [f for f in FORMS[2048] if f[0] == 'span']
        assert len(span) == 4
        base_out, base_nxt = got[span[0]]
        for f in span[1:]:
            out, nxt = got[f]
            assert ds.live(out).tobytes() == ds.live(base_out).tobytes(), (kind, f)
            for k in nxt.dtype.names:                        # (a drift list of one entry: not locked)
                a, b = (nxt[k], base_nxt[k]) if k != 'df' else (nxt[k][..., 0], base_nxt[k][..., 0])
                assert ds.live(a).tobytes() == ds.live(b).tobytes(), (kind, f, k)
            assert (ds.live(nxt['df_len']) == 1).all()
