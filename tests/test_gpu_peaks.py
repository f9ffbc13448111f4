"""GPU: the auxiliary peaks (gpsmi_acq_peaks_dev) against the numpy restatement
(peaks_ref.py), byte for byte.

The surfaces are synthetic and uploaded as they are (no search): small integers, so that equal
values of S in one bin give equal z and ties are exact, and there are many of them -- with sixteen
levels over thousands of lags every pick is a tie that only the first-index rules decide.  One case
takes real rows from Acquisition.deepRows and holds the pick of a single-bin window to the search's
own record."""
import numpy as np
import pytest

import peaks_ref as R
from test_gpu_acq_noncoherent import CFG, _same, _upload

pytestmark = pytest.mark.gpu

CS = (2048, 16368)


@pytest.fixture(scope='module')
def engines():
    from gpsmi.engine import AcqEngine, Config
    es = {cs: AcqEngine(Config(**CFG[cs]), prns=(3, 6)) for cs in CS}
    yield es
    for e in es.values():
        e.close()


_SURF = {}


def surfaces(cs):
    """float32 [3][51][cs] of integers 0..15, the same for every test of a code length."""
    if cs not in _SURF:
        _SURF[cs] = np.random.default_rng(cs).integers(0, 16, (3, 51, cs)).astype(np.float32)
        _SURF[cs].setflags(write=False)
    return _SURF[cs]


def run(e, rows, k, guard, bins, **kw):
    """One call on the host array rows [nsv][nbins][cs]."""
    buf = _upload(np.ascontiguousarray(rows, np.float32))
    try:
        return e.peaks(buf, rows.shape[0], rows.shape[1], k=k, guard_lags=guard, bins=bins, **kw)
    finally:
        buf.free()


def same_as_ref(got, ref):
    _same(got[0], ref[0])
    _same(got[1], ref[1])


def windows(nbins):
    return {1: [None, (0, 0)], 3: [None, (1, 2), (1, 1)], 51: [None, (10, 40), (25, 25)]}[nbins]


@pytest.mark.parametrize('nbins', [1, 3, 51])
@pytest.mark.parametrize('nsv', [1, 3])
@pytest.mark.parametrize('cs', CS)
def test_sweep_equals_restatement(engines, cs, nsv, nbins):
    e = engines[cs]
    rows = np.ascontiguousarray(surfaces(cs)[:nsv, :nbins])
    buf = _upload(rows)
    try:
        for bins in windows(nbins):
            lo, hi = bins or (0, nbins - 1)
            zs = [R.surface_z(S, lo, hi) for S in rows]
            for k in (1, 4, 8):
                for guard in (0, -1, cs // 2):
                    ref = [R.picks_of(S, z, used, k, guard) for S, (z, used) in zip(rows, zs)]
                    got = e.peaks(buf, nsv, nbins, k=k, guard_lags=guard, bins=bins)
                    same_as_ref(got, (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])))
                    assert e.last_ms() > 0
    finally:
        buf.free()


def planted(cs):
    """[1][3][cs]: a background of 0, 1, 2 with equal spikes at lags 5 and 900 in bins 0 and 2 (the
    same rows), bin 1 constant."""
    S = np.zeros((1, 3, cs), np.float32)
    S[0, 0] = S[0, 2] = np.arange(cs) % 3
    S[0, 0, [5, 900]] = S[0, 2, [5, 900]] = 100.0
    S[0, 1] = 7.0
    return S


@pytest.mark.parametrize('cs', CS)
def test_planted_ties_and_skips(engines, cs):
    e = engines[cs]
    S = planted(cs)
    got = run(e, S, 4, -1, None)
    same_as_ref(got, R.peaks(S, 4, -1))
    picks, cols = got
    assert list(picks[0]['lag'][:2]) == [5, 900]               # two equal maxima: the first wins
    assert list(picks[0]['bin'][:2]) == [0, 0]                 # equal z in bins 0 and 2: the smaller
    assert picks[0]['z'][0] == picks[0]['z'][1] and picks[0]['s'][0] == 100.0
    assert np.all(cols[0, :, 1, 1] == 0) and np.all(cols[0, :, 0, 1] == 7.0)      # the constant bin: skipped
    assert np.array_equal(cols[0, 0, 1, 0], picks[0]['z'][0])
    # the window on the constant bin alone, and all rows constant: every pick -1, the columns zero
    for rows, bins in ((S, (1, 1)), (np.full((1, 3, cs), 3.0, np.float32), None)):
        got = run(e, rows, 4, -1, bins)
        same_as_ref(got, R.peaks(rows, 4, -1, bins))
        assert np.all(got[0]['lag'] == -1) and np.all(got[0]['bin'] == -1)
        assert not got[0]['z'].any() and not got[0]['s'].any() and not got[1].any()
    # guard cs / 2 takes every lag: the second pick is -1
    got = run(e, S, 4, cs // 2, None)
    same_as_ref(got, R.peaks(S, 4, cs // 2))
    assert got[0]['lag'][0, 0] == 5 and np.all(got[0]['lag'][0, 1:] == -1)


@pytest.mark.parametrize('cs', CS)
def test_guard_wraps(engines, cs):
    e = engines[cs]
    g = R.default_guard(cs)
    S = (np.arange(cs) % 3).astype(np.float32)[None, None, :].copy()
    S[0, 0, 0], S[0, 0, cs - 1], S[0, 0, cs - g], S[0, 0, cs - g - 1], S[0, 0, 500] = 100.0, 90.0, 85.0, 60.0, 80.0
    got = run(e, S, 3, -1, None)
    same_as_ref(got, R.peaks(S, 3, -1))
    assert list(got[0]['lag'][0]) == [0, 500, cs - g - 1]      # cs - 1 and cs - g lie in the stripe of lag 0
    S[0, 0, 0], S[0, 0, cs - 1] = 90.0, 100.0                  # the other way round
    S[0, 0, g - 1], S[0, 0, g] = 85.0, 60.0
    got = run(e, S, 4, -1, None)
    same_as_ref(got, R.peaks(S, 4, -1))
    assert list(got[0]['lag'][0][:3]) == [cs - 1, 500, g]      # 0 .. g - 1 lie in the stripe of lag cs - 1


@pytest.mark.parametrize('cs', CS)
def test_alone_and_among_others_twice_and_on_the_device(engines, cs):
    from gpsmi.engine import DeviceBuffer, PEAKS_PICK_DTYPE
    e = engines[cs]
    rows = np.ascontiguousarray(surfaces(cs)[:, :3])
    k = 4
    picks, cols = run(e, rows, k, -1, (0, 1))
    for j in range(3):
        same_as_ref(run(e, rows[j:j + 1], k, -1, (0, 1)), (picks[j:j + 1], cols[j:j + 1]))
    d_p, d_c = DeviceBuffer(picks.nbytes), DeviceBuffer(cols.nbytes)
    try:
        again = run(e, rows, k, -1, (0, 1), out_dev=d_p.ptr, cols_dev=d_c.ptr)
        same_as_ref(again, (picks, cols))
        _same(d_p.download(PEAKS_PICK_DTYPE, picks.size).reshape(picks.shape), picks)
        _same(d_c.download(np.float32, cols.size).reshape(cols.shape), cols)
    finally:
        d_p.free()
        d_c.free()
    only, none = run(e, rows, k, -1, (0, 1), cols=False)
    assert none is None
    _same(only, picks)


def test_refusals_leave_the_engine_usable(engines):
    from gpsmi.engine import EngineError
    e = engines[2048]
    rows = np.ascontiguousarray(surfaces(2048)[:1, :3])
    for k, guard, bins in ((0, -1, None), (9, -1, None), (4, -2, None), (4, 1025, None), (4, -1, (2, 1)),
                           (4, -1, (0, 3))):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            run(e, rows, k, guard, bins)
    with pytest.raises(ValueError):                    # a buffer too small never reaches the kernels
        buf = _upload(rows)
        try:
            e.peaks(buf, 2, 3)
        finally:
            buf.free()
    same_as_ref(run(e, rows, 2, -1, None), R.peaks(rows, 2, -1))


@pytest.mark.parametrize('raw', [False, True])
@pytest.mark.parametrize('cs', CS)
def test_real_rows_single_bin_is_the_search_record(cs, raw):
    from deep_ref import deep_scene
    from gpsmi.acquisition import Acquisition
    from gpsmi.engine import Config
    from gpsmi.synth import raw_to_c64
    prns, freqs, n_coh, n_seg = [6, 3], [-200.0, 0.0, 200.0], 1, 2
    data = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.05).block_raw(0, n=n_seg * n_coh * cs)
    acq = Acquisition(Config(**CFG[cs]), raw_u8=raw)
    try:
        tab, rows = acq.deepRows(data if raw else raw_to_c64(data), prns, freqs, n_coh, n_seg)
        try:
            host = rows.download(np.float32, len(prns) * len(freqs) * cs).reshape(len(prns), len(freqs), cs)
            for b in range(len(freqs)):
                picks, cols = acq.engine.peaks(rows, len(prns), len(freqs), k=4, bins=(b, b))
                same_as_ref((picks, cols), R.peaks(host, 4, -1, (b, b)))
                for j in range(len(prns)):
                    assert picks[j, 0]['lag'] == tab[b, j]['argmax'] and picks[j, 0]['bin'] == b
                    assert picks[j, 0]['s'] == tab[b, j]['peak']
            same_as_ref(acq.engine.peaks(rows, len(prns), len(freqs), k=4), R.peaks(host, 4, -1))
        finally:
            rows.free()
    finally:
        acq.engine.close()
