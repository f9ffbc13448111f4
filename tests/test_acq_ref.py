"""The float64 restatement of the acquisition searches (tests/acq_ref.py) itself, without a GPU:
against the project's float32 oracle (acq_table, nc_table, deep_table) at every code length
test_gpu_acq_ref.py uses, on noise-free replicas across the wrap, on the all-zero input, on the deep
rotation, the integer-exact record against direct integer dot products -- and every seeded input of
the GPU file against the GPU file's near-tie caps, so that those hold before a GPU is asked."""
import numpy as np
import pytest

import acq_ref as ar
import gps_oracle as orc

ORACLE_RTOL = 1e-4
LENGTHS = sorted({row[1] for row in ar.MATRIX.values()})


def _small_input(cs, periods, seed):
    lags = ar.peak_lags(cs, 'direct')[0]
    return ar.signal_input(cs, periods, lags, seed)[0]


def _agrees(rec, tab):
    assert np.array_equal(rec['argmax'], tab['argmax'])
    for k in ('peak', 'mean', 'std'):
        np.testing.assert_allclose(rec[k], tab[k], rtol=ORACLE_RTOL)


@pytest.mark.parametrize('cs', LENGTHS)
def test_reference_agrees_with_the_oracles_coherent_table(cs):
    """One small case per code length: acq_ref against orc.acq_table to 1e-4, and oracle_record --
    the same oracle functions with the neighbours kept -- against it too."""
    n_avg = 1 if cs >= 16384 else 2
    iq = _small_input(cs, n_avg, 5 + cs)
    prns, freqs = [1, 9, 37], [0.0, -5000.0, 1250.0]
    rec = ar.acq_ref(iq, freqs, prns, cs, n_avg)
    tab = orc.acq_table(iq, freqs, prns, n_avg, orc.Params(code_samples=cs, n_cyc=n_avg))
    _agrees(rec, tab)
    o = ar.oracle_record(iq, freqs, prns, cs, n_avg)         # (float32 behind the forward transform too)
    _agrees(o, tab)
    np.testing.assert_allclose(o['lo'], rec['lo'], atol=ORACLE_RTOL * rec['rms'].max())
    np.testing.assert_allclose(o['hi'], rec['hi'], atol=ORACLE_RTOL * rec['rms'].max())
    if 2 * cs - 1 <= ar.BIG_N:
        p = ar.oracle_record_padded(iq, freqs, prns, cs, n_avg)
        _agrees(p, tab)
        np.testing.assert_allclose(p['lo'], rec['lo'], atol=ORACLE_RTOL * rec['rms'].max())


@pytest.mark.parametrize('cs', [2048, 16368])
def test_reference_agrees_with_the_oracles_segmented_tables(cs):
    from deep_ref import deep_table
    from test_acq_noncoherent import nc_table
    n_coh, n_seg = 2, 3
    iq = _small_input(cs, n_coh * n_seg, 11 + cs)
    prns, freqs = [1, 20], list(ar.DEEP_BINS[:4])
    p = orc.Params(code_samples=cs, n_cyc=n_coh)
    _agrees(ar.acq_ref(iq, freqs, prns, cs, n_coh, n_seg), nc_table(iq, freqs, prns, n_coh, n_seg, p))
    carrier = n_coh * cs / ar.DEEP_K[cs]
    shifts = ar.deep_shifts(freqs, n_coh, n_seg, cs, carrier)
    assert (shifts[:, 1:] != 0).any()
    rec = ar.acq_ref(iq, freqs, prns, cs, n_coh, n_seg, shifts)
    tab = deep_table(iq, freqs, prns, n_coh, n_seg, p, carrier_hz=carrier)
    _agrees(rec, tab)
    _agrees(ar.oracle_record(iq, freqs, prns, cs, n_coh, n_seg, shifts), tab)


@pytest.mark.parametrize('cs', [1024, 2048, 1040])
def test_rolled_noise_free_replica_peaks_at_its_roll(cs):
    """lo and hi are taken across the wrap at rolls 0 and cs - 1."""
    rep = ar.replica(5, cs)
    full = ar.corr_mag(np.fft.fft(rep), np.fft.fft(rep))            # the autocorrelation, peak at 0
    for d in (0, 1, cs // 2, cs - 1):
        iq = (0.5 * np.roll(rep, d)).astype(np.complex64)
        r = ar.acq_ref(iq, [0.0], [5], cs, 1)[0, 0]
        assert r['argmax'] == d
        np.testing.assert_allclose([r['lo'], r['peak'], r['hi']], 0.5 * full[[cs - 1, 0, 1]], rtol=1e-6)
        S = ar.rotated_mean([ar.corr_mag(np.fft.fft(ar.fold(iq, 0.0, cs, 1)), np.fft.fft(rep))])
        assert r['lo'] == S[(d - 1) % cs] and r['hi'] == S[(d + 1) % cs]
        direct = abs(np.dot(iq.astype(np.complex128), np.roll(rep, (d + 1) % cs)))
        np.testing.assert_allclose(r['hi'], direct, rtol=1e-9)


def test_all_zero_input_gives_the_zero_record():
    for cs, n_seg, shifts in ((2048, 1, None), (1040, 1, None), (2048, 2, np.array([[0, 5]]))):
        r = ar.acq_ref(np.zeros(2 * cs, np.complex64), [1250.0], [3], cs, 1, n_seg, shifts)[0, 0]
        assert tuple(r[k] for k in ar.FIELDS) == (0, 0, 0, 0, 0, 0)
        assert r['gap'] == 0 and not any(np.isnan(r[k]) for k in r.dtype.names)
    # no raw byte decodes to exactly 0 (127.5 is not a byte): there is no raw all-zero input
    assert not (ar.decode_u8(np.arange(256, dtype=np.uint16)).real == 0).any()


def test_deep_rotation_agrees_with_roll():
    cs = 2048
    rng = np.random.default_rng(3)
    c0, c1 = rng.random(cs), rng.random(cs)
    for m in (0, 1, cs - 1):
        S = ar.rotated_mean([c0, c1], [0, m])
        assert np.array_equal(S, (c0 + np.roll(c1, -m)) / 2)
        i = np.arange(cs)
        assert np.array_equal(S, (c0 + c1[(i + m) % cs]) / 2)


def test_deep_cases_hold_every_kind_of_shift():
    """2048: no shift, 1, cs - 1 and one above 1792 (the rotated read wraps in the last 256-lane
    row); 16368: one that crosses a layout row of 1023 lags with a carry."""
    for search in (('deep', 1, 2), ('deep', 5, 3)):
        m = ar.case_search('fft2048_seg', search)[4]
        assert (m[:, 0] == 0).all()
        assert {0, 1, 2047} <= set(m[:, 1].tolist()) and any(1792 < v < 2047 for v in m[:, 1])
    m = ar.case_search('pfa16368', ('deep', 2, 3))[4]
    assert any(v > 1023 and v % 1023 > 0 for v in m[:, 1]) and 0 in m[:, 1] and (m[:, 2] != m[:, 1]).any()


@pytest.mark.parametrize('cs', [1024, 1040, 16400])
def test_exact_integer_record_equals_integer_dot_products(cs):
    reps = ar.integer_replicas(cs, 90 + cs)
    for n_coh in (1, 4):
        iq, sats = ar.integer_input(cs, n_coh, reps, 91 + cs)
        assert np.abs(iq.real).max() * cs * n_coh < 2 ** 24
        for prn in (1, 9, 4):
            r, S = ar.exact_integer_record(iq, prn, cs, n_coh, reps, surface=True)
            lags = [0, 1, 2, 511, 512, 1022, 1023, 1024 % cs, 1025 % cs, cs // 2, cs - 2, cs - 1]
            for lag in lags:
                re, im = ar.integer_dot(iq, prn, cs, n_coh, reps, lag)
                assert S[lag] == np.hypot(re, im) / n_coh, (prn, n_coh, lag)
        for prn, _, lag, a in sats:
            r = ar.exact_integer_record(iq, prn, cs, n_coh, reps)
            assert r['argmax'] == lag and r['peak'] > 0.7 * a * cs
    hi, lo = ar.tie_lags(cs)
    x = ar.tie_input(cs, 1, reps, 20, (hi, lo))
    r, S = ar.exact_integer_record(x, 20, cs, 1, reps, surface=True)
    assert lo < hi and r['argmax'] == lo and S[lo] == S[hi] and r['gap'] == 0


def test_present_replicas_peak_where_they_were_put():
    """Coherent 1-ms searches of every row: the strong PRNs peak at lag 0, cs - 1 and on both sides
    of the path's internal boundary, in the bin of their Doppler."""
    for name, (path, cs, _, searches) in ar.MATRIX.items():
        coh = [s for s in searches if s[0] == 'coh']
        if not coh:
            continue
        prns, freqs = ar.case_search(name, coh[0])[:2]
        for which, (_, sats) in enumerate(ar.case_inputs(name)):
            rec = ar.case_reference(name, coh[0], which)[0]
            for prn, f, lag, a, strong in sats:
                if strong and f in freqs and prn in prns:
                    assert rec['argmax'][freqs.index(f), prns.index(prn)] == lag, (name, prn, lag)


def test_every_gpu_input_stays_under_the_near_tie_caps():
    """Per test of test_gpu_acq_ref.py (a row of the matrix over its searches and inputs): the cells
    whose two largest float64 lags are within 1e-4 of each other number no more than the cap."""
    for name, (_, _, _, searches) in ar.MATRIX.items():
        cells = near = 0
        for search in searches:
            for which in range(len(ar.case_inputs(name))):
                rec = ar.case_reference(name, search, which)[0]
                cells += rec.size
                near += int((rec['gap'] <= ar.NEAR_TIE).sum())
        assert near <= ar.excused_cap(cells), (name, near, cells)
    # the second chunk's last bin, and the integer inputs on the 32768-pair path: no cell excused
    rec = ar.acq_ref(ar.chunk_input(), ar.CHUNK_BINS[-1:], ar.CHUNK_PRNS, ar.CHUNK_CS, 1)
    assert (rec['gap'] > ar.NEAR_TIE).all()
    for cs in ar.INTEGER_BIG:
        reps, iq, _, n_avgs = ar.integer_case(cs)
        for n_avg in n_avgs:
            assert (ar.acq_ref(iq, [0.0], ar.PRNS, cs, n_avg, reps=reps)['gap'] > ar.NEAR_TIE).all(), (cs, n_avg)
    assert ar.excused_cap(99) == 0 and ar.excused_cap(100) == 1 and ar.excused_cap(518) == 5
