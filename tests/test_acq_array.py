"""CPU: the array search (gpsmi_acq_search_array) without a GPU -- the plan's
argument checks, the float64 restatement's own properties (tests/array_ref.py), and the seeded inputs
of test_gpu_acq_array.py held to "no near tie in float64", so that the GPU file can ask for exact
argmaxes everywhere."""
import numpy as np
import pytest

import acq_ref as ar
import array_ref as R


# ---- the plan -------------------------------------------------------------------------------------

def _plan(**kw):
    from gpsmi.engine import search_array_plan
    a = dict(code_samples=2048, n=250 * 4 * 2048, antennas=4, nbins=51, n_coh=4, n_seg=250)
    a.update(kw)
    return search_array_plan(**a)


def test_plan_accepts_and_sizes():
    """The flagship shape: 250 x 4 ms over four antennas are 16 MiB of spectra a bin, so 32 bins a
    launch, and the 51 bins take two."""
    scratch, nbc = _plan()
    assert nbc == 32 and scratch == 32 * 4 * 250 * 2048 * 8
    assert _plan(antennas=2) == (51 * 2 * 250 * 2048 * 8, 51)
    assert _plan(antennas=3, nbins=3, n_coh=1, n_seg=5, n=5 * 2048) == (3 * 3 * 5 * 2048 * 8, 3)
    assert _plan(nbins=0) == (0, 0)
    assert R.CHUNK_N_SEG * R.CHUNK_N_COH * 2048 * 8 * R.CHUNK_A * 32 == 512 << 20
    assert _plan(antennas=R.CHUNK_A, nbins=len(R.CHUNK_BINS), n_coh=R.CHUNK_N_COH, n_seg=R.CHUNK_N_SEG,
                 n=R.CHUNK_N_SEG * 2048)[1] == 32 < len(R.CHUNK_BINS)


@pytest.mark.parametrize('kw', [
    dict(antennas=1), dict(antennas=5), dict(antennas=0), dict(n=(1 << 40) // 4 + 1), dict(nbins=-1),
    dict(nbins=65536), dict(n_coh=0), dict(n_coh=65), dict(n_seg=0), dict(n_seg=65536),
    dict(n=250 * 4 * 2048 - 1), dict(carrier_hz=0.0), dict(carrier_hz=-1.0), dict(carrier_hz=float('nan')),
    dict(f_offset=float('inf')), dict(code_samples=1000)])
def test_plan_refuses_bad_arguments(kw):
    from gpsmi.engine import EngineError
    with pytest.raises(EngineError, match=r'\(-1\)'):
        _plan(**kw)


@pytest.mark.parametrize('kw', [
    dict(code_samples=16368, n=250 * 4 * 16368), dict(code_samples=4096, n=250 * 4 * 4096),
    dict(antennas=4, n_coh=1, n_seg=8193, n=8193 * 2048), dict(antennas=2, n_coh=1, n_seg=16385, n=16385 * 2048)])
def test_plan_reports_what_is_unsupported(kw):
    """Other code lengths, and one bin's segments over all antennas beyond 512 MiB: A n_seg 2048 8
    bytes, 8192 segments at four antennas and 16384 at two still fit."""
    from gpsmi.engine import EngineError
    with pytest.raises(EngineError, match=r'\(-5\)'):
        _plan(**kw)
    if 'n_seg' in kw:
        kw = dict(kw, n_seg=kw['n_seg'] - 1)
        assert _plan(**kw)[1] == 1


def test_plan_limit_of_n_times_antennas():
    assert _plan(n=(1 << 40) // 4)[1] == 32


# ---- the restatement's own properties ---------------------------------------------------------------

@pytest.fixture(scope='module')
def small():
    """Four antennas, 2 x 3 periods, two bins (one shifting), two PRNs."""
    c64 = R.case_rows(4, 2, 3)[1]
    freqs, prns = [0.0, -37.5], [9, 4]
    return c64, freqs, prns, R.shifts(2, 3, freqs)


def _one_row(x, f, prns, m):
    """[nsv][cs]: (1 / n_seg) sum_s |c_s|^2 of a single row, segments rotated, from acq_ref's parts."""
    out = []
    for p in prns:
        rs = np.conj(np.fft.fft(ar.replica(p, 2048)))
        acc = np.zeros(2048)
        for s in range(3):
            c = np.fft.ifft(np.fft.fft(ar.fold(x, f, 2048, 2, s)) * rs)
            acc += np.roll(np.abs(c) ** 2, -int(m[s]))
        out.append(acc / 3)
    return np.array(out)


@pytest.mark.parametrize('A', [2, 3, 4])
def test_rows_of_zeros_leave_row_0_over_A(small, A):
    c64, freqs, prns, m = small
    x = np.zeros((A, c64.shape[1]), np.complex64)
    x[0] = c64[0]
    T = R.array_surfaces(x, freqs, prns, 2, 3, m)
    for b, f in enumerate(freqs):
        np.testing.assert_allclose(T[b], _one_row(c64[0], f, prns, m[b]) / A, rtol=1e-12, atol=0)


@pytest.mark.parametrize('A', [2, 3, 4])
def test_equal_rows_give_A_times_the_mean_power(small, A):
    c64, freqs, prns, m = small
    x = np.stack([c64[1]] * A)
    T = R.array_surfaces(x, freqs, prns, 2, 3, m)
    for b, f in enumerate(freqs):
        np.testing.assert_allclose(T[b], A * _one_row(c64[1], f, prns, m[b]), rtol=1e-12, atol=0)


def test_permuting_rows_changes_nothing(small):
    c64, freqs, prns, m = small
    T = R.array_surfaces(c64, freqs, prns, 2, 3, m)
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        np.testing.assert_allclose(R.array_surfaces(c64[perm], freqs, prns, 2, 3, m), T, rtol=1e-12, atol=0)
    # ... and a common phase, or a phase per antenna, does not either
    turned = c64 * np.exp(1j * np.array([0.4, 1.7, 2.9, 5.1]))[:, None]
    np.testing.assert_allclose(R.array_surfaces(turned, freqs, prns, 2, 3, m), T, rtol=1e-9, atol=0)


def test_float32_restatement_follows_the_float64_one(small):
    c64, freqs, prns, m = small
    T = R.array_surfaces(c64, freqs, prns, 2, 3, m)
    T32 = R.array_f32(c64, freqs, prns, 2, 3, m)
    dev = R.row_deviation(T32, T)
    assert 0 < dev.max() < 1e-5, dev
    assert np.array_equal(R.records_f32(T32)['argmax'], R.records(T)['argmax'])


def test_raw_rows_are_their_decode():
    from gpsmi.synth import raw_to_c64
    raw, c64 = R.planted_rows(3, 20)
    assert raw.dtype == np.uint16 and np.array_equal(np.stack([raw_to_c64(r) for r in raw]), c64)


# ---- the GPU file's cases: shifts and near ties -----------------------------------------------------

def test_shifts_of_the_gpu_cases():
    """0 for the 0 Hz bin; non-zero and different per segment elsewhere; one bin wraps from 2047
    down, the other counts up through its ties."""
    for n_coh in (1, 4):
        m = R.shifts(n_coh, 5)
        assert (m[0] == 0).all()
        assert list(m[1]) == [0, 2047, 2046, 2045, 2044]
        assert list(m[2]) == [0, 2, 3, 4, 6]             # rint(1.5 s): 1.5 and 4.5 go to even
    m = ar.deep_shifts(R.CHUNK_BINS, R.CHUNK_N_COH, R.CHUNK_N_SEG, 2048, f_offset=R.CHUNK_OFFSET)
    assert len({tuple(r) for r in m}) == len(R.CHUNK_BINS) and m[32:, 1:].any(axis=1).all()


@pytest.mark.parametrize('A', R.ANTENNAS)
def test_gpu_cases_have_no_near_tie_and_show_their_planted_codes(A):
    for n_coh, n_seg in R.SHAPES:
        T, rec, T32, rec32 = R.case_reference(A, n_coh, n_seg)
        assert (rec['gap'] > ar.NEAR_TIE).all(), (A, n_coh, n_seg, rec['gap'])
        assert np.array_equal(rec32['argmax'], rec['argmax'])
        for prn, f, lag in R.PLANTED:
            b, j = R.BINS.index(f), R.PRNS.index(prn)
            if f == 0.0 or n_seg == 1:               # (elsewhere the segments are added apart)
                assert rec[b, j]['argmax'] == lag, (A, n_coh, n_seg, prn)


def test_second_launch_case_has_no_near_tie():
    T, rec, T32, rec32 = R.chunk_reference()
    assert (rec['gap'] > ar.NEAR_TIE).all(), rec['gap']
    assert np.array_equal(rec32['argmax'], rec['argmax'])
    assert 689 <= rec[0, 0]['argmax'] <= 700                # the ridge of the planted code
    assert (rec[0, 0]['peak'] - rec[0, 0]['mean']) / rec[0, 0]['std'] > 8       # (a detection at corr_min 8)


# ---- the options of measure / snapshot_fix ----------------------------------------------------------

def test_measure_option_rules():
    """array=True needs antennas = 2 .. 4 and goes with neither spoof nor cancel; antennas without
    spoof and without array raises as before.  (All refused before anything touches a GPU.)"""
    import types
    from gpsmi import snapshot as S
    from gpsmi.engine import Config
    acq = types.SimpleNamespace(cfg=Config())
    x = np.zeros((4, 100), np.complex64)
    for kw, word in ((dict(array=True), 'antennas'), (dict(array=True, antennas=4, spoof=True), 'spoof'),
                     (dict(array=True, antennas=4, cancel=True), 'cancel'), (dict(array=True, antennas=4, cancel=40.0), 'cancel'),
                     (dict(array=True, antennas=5), '2 .. 4'), (dict(array=True, antennas=1), '2 .. 4'),
                     (dict(antennas=4), 'spoof=True')):
        with pytest.raises(ValueError, match=word):
            S.measure(acq, x, **kw)
    for kw in (dict(array=True), dict(array=True, antennas=4, spoof=True), dict(array=True, antennas=4, beams=True),
               dict(array=True, antennas=4, collective=True, pos=np.zeros(3)), dict(antennas=4)):
        with pytest.raises(ValueError):
            S.snapshot_fix(acq, x, {}, 0.0, **kw)


# ---- the scene (tests/array_truth.py) ---------------------------------------------------------------

def test_scene_holds_its_conditions_on_the_restatement():
    """Antenna 0's deep search leaves at least four of the eight below corr_min - 1; the array's T puts
    all eight above corr_min + 1 at the true lag; no absent PRN comes within 1 of corr_min on either.
    (AMP is the starting value of the issue, DEEP_AMP 10^(-5/20): nothing had to be moved.)"""
    import array_truth as AT
    assert AT.AMP == AT.START_AMP and abs(AT.AMP - 0.0025868) < 1e-7
    out, absent = AT.restated()
    print('\nprn   z antenna 0   z array   z array at the true lag   argmax   true lag')
    for prn, d in out.items():
        print(f"{prn:3d} {d['z0']:10.2f} {d['zT']:10.2f} {d['zT_true']:14.2f} {d['lagT']:16d} {d['lag']:10.2f}")
    print('absent PRNs: antenna 0 %.2f, array %.2f' % absent)
    assert len(out) == 8
    assert sum(d['z0'] < AT.CORR_MIN - 1 for d in out.values()) >= 4
    assert all(d['zT_true'] > AT.CORR_MIN + 1 for d in out.values())
    assert all(abs(d['lagT'] - d['lag']) <= 1 for d in out.values())
    assert absent[0] < AT.CORR_MIN - 1 and absent[1] < AT.CORR_MIN - 1
