"""GPU: the array search (gpsmi_acq_search_array[_dev], csrc/gpsmi_acq_array.h) against its float64
restatement (tests/array_ref.py) at the smallest shapes at which it can go wrong: A = 2, 3, 4 antennas,
n_coh 1 and 4 (both spectrum kernels), n_seg 1, 2 and 5, 3 PRNs x 3 bins whose shifts are 0, wrap
from 2047 down, and count up through two ties to even -- non-zero and different per segment --,
complex64 and raw input, host and device entry points, and one call whose bins take two launches.

Per A, over the cells of all six shapes:
  - argmax equals the float64 one (test_acq_array.py holds the inputs to "no near tie in float64"
    without a GPU, so no cell is excused);
  - peak, lo, hi, mean as |value - ref| / rms, std relatively, and every lag of the rows as
    |value - ref| / rms of the row, are within 4 x the worst deviation of the float32 numpy
    restatement (array_ref.array_f32) from the float64 one over the same cells: the same operation
    in another legal rounding order (the factor is test_gpu_acq_ref.py's).
Bytewise: host entry = device entry; raw input = its complex64 decode; a cell does not depend on what
shares the call, nor on the launch it falls into; the rows are what the records are statistics of;
AcqEngine.peaks over the rows is peaks_ref over the same rows.
The figures of an MI355X run (kernel error over bound per field) are in DESIGN.md 4.2s."""
import numpy as np
import pytest

import acq_ref as ar
import array_ref as R
from test_gpu_acq_noncoherent import _same, _upload

pytestmark = pytest.mark.gpu

FACTOR = 4
ALL_PRNS = tuple(sorted(set(R.PRNS + R.CHUNK_PRNS)))


@pytest.fixture(scope='module')
def engines():
    """{raw?: a 2048 handle of that input format}"""
    from gpsmi.engine import AcqEngine, Config
    es = {raw: AcqEngine(Config(code_samples=2048, n_cyc=32), prns=ALL_PRNS) for raw in (False, True)}
    es[True].set_input_format(True)
    yield es
    for e in es.values():
        e.close()


def _rows_buffer(nsv, nbins):
    from gpsmi.engine import DeviceBuffer
    return DeviceBuffer(nsv * nbins * R.CS * 4)


def _fetch_rows(buf, nsv, nbins):
    return buf.download(np.float32, nsv * nbins * R.CS).reshape(nsv, nbins, R.CS)


def _records(tab, nbr):
    got = np.zeros(tab.shape, ar.REC_DTYPE)
    for k in ('argmax', 'peak', 'mean', 'std'):
        got[k] = tab[k]
    got['lo'], got['hi'] = nbr[..., 0], nbr[..., 1]
    for k in ar.FIELDS:
        assert np.isfinite(got[k]).all(), k
    return got


def _rows_hold_records(rows, tab):
    """argmax is the first index of a row's maximum and peak its value, exactly."""
    for j, b in np.ndindex(rows.shape[:2]):
        assert int(np.argmax(rows[j, b])) == tab[b, j]['argmax'], (j, b)
        assert rows[j, b].max() == tab[b, j]['peak'], (j, b)


def _every_entry(engines, A, n_coh, n_seg, prns=R.PRNS, bins=R.BINS, **kw):
    """One search through every entry point and input format -> (table, neighbours, rows
    [nsv][nbins][cs]), all of them the same bytes."""
    raw, c64 = R.case_rows(A, n_coh, n_seg)
    n = c64.shape[1]
    e, er = engines[False], engines[True]
    kw = dict(carrier_hz=R.carrier(n_coh), **kw)
    tab, nbr = e.search_array(c64, A, prns, bins, n_coh, n_seg, nbr=True, **kw)
    assert e.last_ms() > 0
    _same(e.search_array(c64, A, prns, bins, n_coh, n_seg, **kw), tab)
    tab_r, nbr_r = er.search_array(raw, A, prns, bins, n_coh, n_seg, nbr=True, **kw)
    _same(tab_r, tab)
    _same(nbr_r, nbr)
    out = []
    for eng, data in ((e, c64), (er, raw)):
        buf, rbuf = _upload(data), _rows_buffer(len(prns), len(bins))
        try:
            _same(eng.search_array((buf.ptr, n), A, prns, bins, n_coh, n_seg, **kw), tab)
            _same(eng.search_array((buf.ptr, n), A, prns, bins, n_coh, n_seg, rows=rbuf, **kw), tab)
            out.append(_fetch_rows(rbuf, len(prns), len(bins)))
        finally:
            buf.free()
            rbuf.free()
    _same(out[0], out[1])
    _rows_hold_records(out[0], tab)
    return tab, nbr, out[0]


@pytest.mark.parametrize('A', R.ANTENNAS)
def test_against_float64(engines, A):
    gots, refs, f32s, row_dev, row_dev32 = [], [], [], [], []
    for n_coh, n_seg in R.SHAPES:
        tab, nbr, rows = _every_entry(engines, A, n_coh, n_seg)
        T, rec, T32, rec32 = R.case_reference(A, n_coh, n_seg)
        got = _records(tab, nbr)
        assert (rec['gap'] > ar.NEAR_TIE).all()
        assert np.array_equal(got['argmax'], rec['argmax']), (A, n_coh, n_seg, got['argmax'], rec['argmax'])
        gots.append(got.ravel())
        refs.append(rec.ravel())
        f32s.append(rec32.ravel())
        row_dev.append(R.row_deviation(rows.transpose(1, 0, 2), T).ravel())
        row_dev32.append(R.row_deviation(T32, T).ravel())
    got, ref, f32 = (np.concatenate(x) for x in (gots, refs, f32s))
    assert np.array_equal(f32['argmax'], ref['argmax'])
    dev, dev32 = ar.deviations(got, ref), ar.deviations(f32, ref)
    worst = {k: float(np.max(dev[k])) for k in ar.METRICS}
    bound = {k: FACTOR * float(np.max(dev32[k])) for k in ar.METRICS}
    worst['rows'], bound['rows'] = float(np.max(np.concatenate(row_dev))), FACTOR * float(np.max(np.concatenate(row_dev32)))
    assert all(v > 0 for v in bound.values()), bound
    print(f'\nA = {A}: {ref.size} cells; kernel error, bound (4 x float32 numpy), ratio')
    for k in worst:
        print(f'    {k:<5} {worst[k]:>10.3e} {bound[k]:>10.3e} {worst[k] / bound[k]:>7.3f}')
    for k in worst:
        assert worst[k] <= bound[k], (A, k, worst[k], bound[k])


def test_a_cell_does_not_depend_on_what_shares_the_call(engines):
    A, n_coh, n_seg = 3, 4, 5
    c64 = R.case_rows(A, n_coh, n_seg)[1]
    e = engines[False]
    kw = dict(carrier_hz=R.carrier(n_coh), nbr=True)
    tab, nbr, rows = _every_entry(engines, A, n_coh, n_seg)
    for b, f in enumerate(R.BINS):
        for j, p in enumerate(R.PRNS):
            one, on = e.search_array(c64, A, [p], [f], n_coh, n_seg, **kw)
            _same(one, tab[b:b + 1, j:j + 1])
            _same(on, nbr[b:b + 1, j:j + 1])
    rev, rn = e.search_array(c64, A, R.PRNS[::-1], R.BINS[::-1], n_coh, n_seg, **kw)
    _same(rev[::-1, ::-1], tab)
    _same(rn[::-1, ::-1], nbr)
    # the rows of a single-cell call are the cell's rows of the whole call
    buf, rbuf = _upload(c64), _rows_buffer(1, 1)
    try:
        e.search_array((buf.ptr, c64.shape[1]), A, [R.PRNS[2]], [R.BINS[1]], n_coh, n_seg, rows=rbuf,
                       carrier_hz=R.carrier(n_coh))
        _same(_fetch_rows(rbuf, 1, 1)[0, 0], rows[2, 1])
    finally:
        buf.free()
        rbuf.free()


def test_bins_in_a_second_launch(engines):
    """34 bins of 512 segments over two antennas: 32 bins a launch (the plan says so), bins 32 and 33
    in a second one.  Their records and rows are those of calls of their own, byte for byte, and the
    last bin holds to the float64 restatement like every other cell."""
    from gpsmi.engine import search_array_plan
    A, n_coh, n_seg, bins, prns = R.CHUNK_A, R.CHUNK_N_COH, R.CHUNK_N_SEG, list(R.CHUNK_BINS), list(R.CHUNK_PRNS)
    raw, c64 = R.chunk_rows()
    n = raw.shape[1]
    assert search_array_plan(2048, n, A, len(bins), n_coh, n_seg)[1] == 32
    er = engines[True]
    kw = dict(f_offset=R.CHUNK_OFFSET)
    buf, rbuf, rone = _upload(raw), _rows_buffer(len(prns), len(bins)), _rows_buffer(len(prns), 1)
    try:
        whole = er.search_array((buf.ptr, n), A, prns, bins, n_coh, n_seg, rows=rbuf, **kw)
        rows = _fetch_rows(rbuf, len(prns), len(bins))
        _rows_hold_records(rows, whole)
        for b in (0, 31, 32, 33):
            one = er.search_array((buf.ptr, n), A, prns, bins[b:b + 1], n_coh, n_seg, rows=rone, **kw)
            _same(one, whole[b:b + 1])
            _same(_fetch_rows(rone, len(prns), 1)[:, 0], rows[:, b])
        host, hn = er.search_array(raw, A, prns, bins, n_coh, n_seg, nbr=True, **kw)
        _same(host, whole)
    finally:
        for x in (buf, rbuf, rone):
            x.free()
    T, rec, T32, rec32 = R.chunk_reference()
    got = _records(host[33:], hn[33:])
    assert (rec['gap'] > ar.NEAR_TIE).all() and np.array_equal(got['argmax'], rec['argmax'])
    dev, dev32 = ar.deviations(got, rec), ar.deviations(rec32, rec)
    rd, rd32 = R.row_deviation(rows[:, 33:].transpose(1, 0, 2), T).max(), R.row_deviation(T32, T).max()
    print(f'\nsecond launch, last bin: rows {rd:.3e} against {FACTOR * rd32:.3e}')
    assert rd <= FACTOR * rd32
    for k in ar.METRICS:
        print(f'    {k:<5} {dev[k].max():>10.3e} {FACTOR * dev32[k].max():>10.3e}')
        assert dev[k].max() <= FACTOR * dev32[k].max(), k


def test_peaks_over_array_rows(engines):
    """gpsmi_acq_peaks_dev takes the rows as it takes the deep search's."""
    import peaks_ref as PR
    A, n_coh, n_seg = 4, 4, 5
    c64 = R.case_rows(A, n_coh, n_seg)[1]
    e = engines[False]
    buf, rbuf = _upload(c64), _rows_buffer(len(R.PRNS), len(R.BINS))
    try:
        e.search_array((buf.ptr, c64.shape[1]), A, R.PRNS, R.BINS, n_coh, n_seg, rows=rbuf,
                       carrier_hz=R.carrier(n_coh))
        rows = _fetch_rows(rbuf, len(R.PRNS), len(R.BINS))
        picks, cols = e.peaks(rbuf, len(R.PRNS), len(R.BINS), k=4)
    finally:
        buf.free()
        rbuf.free()
    ref = PR.peaks(rows, 4, -1)
    _same(picks, ref[0])
    _same(cols, ref[1])
    assert picks[0, 0]['lag'] == 2047 and picks[0, 0]['bin'] == 0        # PRN 9's planted code


def test_what_is_refused(engines):
    from gpsmi.engine import AcqEngine, Config, EngineError
    e = engines[False]
    raw, c64 = R.case_rows(4, 1, 2)
    for A in (1, 5):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.search_array(np.zeros((A, c64.shape[1]), np.complex64), A, R.PRNS, R.BINS, 1, 2)
    with pytest.raises(ValueError):
        e.search_array(c64, 3, R.PRNS, R.BINS, 1, 2)                        # four rows handed over as three
    with pytest.raises(TypeError):
        e.search_array(raw, 4, R.PRNS, R.BINS, 1, 2)
    for kw in (dict(carrier_hz=0.0), dict(f_offset=float('nan'))):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.search_array(c64, 4, R.PRNS, R.BINS, 1, 2, **kw)
    with pytest.raises(EngineError, match=r'\(-1\)'):
        e.search_array(c64, 4, R.PRNS, R.BINS, 1, 3)                        # rows too short
    with pytest.raises(EngineError, match=r'\(-1\)'):
        e.search_array(c64, 4, R.PRNS, [0.0, float('inf')], 1, 2)
    with pytest.raises(EngineError, match=r'\(-3\)'):
        e.search_array(c64, 4, [11], R.BINS, 1, 2)                          # no replica set for PRN 11
    _same(e.search_array(c64, 4, R.PRNS, R.BINS, 1, 2, carrier_hz=R.carrier(1)),
          engines[True].search_array(raw, 4, R.PRNS, R.BINS, 1, 2, carrier_hz=R.carrier(1)))
    long_ = AcqEngine(Config(code_samples=16368, n_cyc=8), prns=(9,))
    try:
        x = np.zeros((2, 2 * 16368), np.complex64)
        with pytest.raises(EngineError, match=r'\(-5\)'):
            long_.search_array(x, 2, [9], [0.0], 1, 2)
    finally:
        long_.close()
