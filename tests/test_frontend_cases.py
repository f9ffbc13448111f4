"""The pinned front-end cases without a GPU (tests/fe_cases.py): every case lands in the planner class
it is there for, by gpsmi_fe_design and the restated workgroup rule (fe_cases.plan_shape, to be kept
in step with the end of fe_plan in csrc/gpsmi_fe.hip: the library exposes neither R nor the LDS
bytes); the outer taps are large enough for a dropped one to show; the configuration that fits no
LDS is refused; and the numpy restatement (tests/fe_ref.py), to which the GPU is held, reproduces
single table entries on a unit impulse."""
import ctypes as C

import numpy as np
import pytest

import fe_cases as FC
import fe_ref as R


def _design(c):
    from gpsmi import frontend
    return frontend.design(c['fs_in'], c['fs_out'], c['fmt'], c['if_hz'], c['conjugate'], c['passband_hz'],
                           c['atten_db'])


def test_output_rate_is_the_engine_rate():
    from gpsmi.engine import Config
    assert Config(code_samples=FC.FS_OUT // 1000).sample_rate == FC.FS_OUT


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_case_lands_in_its_class(name):
    c = FC.CASES[name]
    K, L, T = _design(c)
    P, Q = FC.ratio(c)
    shape = FC.plan_shape(K, L, P, Q)
    assert shape is not None
    r, lds = shape
    print(f'{name}: K {K} L {L} P {P} Q {Q} R {r} LDS {lds} B')
    assert r == c['R'], (name, K, L, r, lds)
    assert (lds > FC.LDS_BUDGET) == c['lds_hi'] and lds <= FC.LDS_MAX, (name, K, L, r, lds)
    if r > 64:                                         # (the next size up did not fit)
        assert lds <= FC.LDS_BUDGET
    if r < 256:
        tab = ((L + 1) * K + 1) & ~1
        assert 4 * tab + 8 * ((2 * r - 1) * P // Q + 1 + K) > FC.LDS_BUDGET
    # the input of the tests holds more than one workgroup and is small
    n_in = FC.n_input(K, P, Q, r)
    assert R.complete(K, P, Q, n_in) >= 3 * r + 5 and n_in <= 300_000
    if c['outer'] is not None:
        big = np.abs(T).max()
        # tap 0 is largest in row 0 (h(K/2 - 1)) and 0 in row L; tap K - 1 the other way round
        assert np.abs(T[0, 0]) >= c['outer'] * big and np.abs(T[L, K - 1]) >= c['outer'] * big, \
            (name, T[0, 0] / big, T[L, K - 1] / big)
        assert T[0, K - 1] == 0 and T[L, 0] == 0


def test_case_relations():
    """What the table says of one case in terms of another."""
    cs = FC.CASES
    for name in ('conj', 'wrap'):
        assert _design(cs[name])[:2] == _design(cs['lo'])[:2]
        assert np.array_equal(_design(cs[name])[2], _design(cs['lo'])[2])
    assert cs['wrap']['if_hz'] > cs['wrap']['fs_in']
    assert R.phase_inc(cs['wrap']['if_hz'], cs['wrap']['fs_in']) == R.phase_inc(312_500.0, 4_000_000)
    for name in ('near1', 'odd'):
        P, Q = FC.ratio(cs[name])
        assert np.gcd(P, Q) == 1 and min(P, Q) >= 2_000_000, (name, P, Q)
    P, Q = FC.ratio(cs['near1'])
    assert P < Q
    assert 0.5 < cs['up']['fs_in'] / cs['up']['fs_out'] < 0.54
    assert cs['negif']['fmt'] == 'r8' and cs['negif']['if_hz'] < 0
    assert {c['fmt'] for c in cs.values()} == set(R.FMT)
    for name in FC.IMPULSE_CASES:
        assert cs[name]['fmt'] == 'c64' and cs[name]['if_hz'] == 0 and not cs[name]['conjugate']
    # one impulse case interpolates between two phase rows (mu != 0); where Q divides L it never does
    K, L, _ = _design(cs['oddc'])
    P, Q = FC.ratio(cs['oddc'])
    assert (K, L) == _design(cs['odd'])[:2] and sum((n * P % Q) * L % Q != 0 for n in range(1, 100)) > 90
    assert all((n * 125 % 64) * 64 % 64 == 0 for n in range(100))


def test_configuration_that_fits_no_lds_is_refused():
    from gpsmi import frontend
    c = FC.REFUSED
    lib = frontend._lib.load()
    cfg = frontend.fe_cfg(c['fs_in'], c['fs_out'], c['fmt'], c['if_hz'], c['conjugate'], c['passband_hz'],
                          c['atten_db'], 1024)
    k, ph = C.c_int(), C.c_int()
    assert lib.gpsmi_fe_design(C.byref(cfg), C.byref(k), C.byref(ph), None) == -5      # GPSMI_E_UNSUPPORTED
    assert 'do not fit the LDS' in lib.gpsmi_last_error().decode()
    h = C.c_void_p(0xBEEF)
    assert lib.gpsmi_fe_create(C.byref(cfg), C.byref(h)) == -5 and h.value is None
    assert 'do not fit the LDS' in lib.gpsmi_last_error().decode()


@pytest.mark.parametrize('name', FC.IMPULSE_CASES)
def test_restatement_on_a_unit_impulse(name):
    """fe_ref.run on a 1.0 at i0 equals the interpolated table entry computed from (n, i0) alone."""
    c = FC.CASES[name]
    K, L, T = _design(c)
    P, Q = FC.ratio(c)
    r = FC.plan_shape(K, L, P, Q)[0]
    n_in = FC.n_input(K, P, Q, r)
    for i0 in FC.impulse_positions(K, P, Q, r):
        x = np.zeros(n_in, dtype=np.complex64)
        x[i0] = 1.0
        y = R.run(x, c, K, L, T)
        want, hit = FC.impulse_expected(K, L, T, P, Q, i0, len(y))
        assert hit.any() and not hit.all()
        assert np.abs(y - want).max() <= 1e-12, (name, i0)
        assert (y[~hit] == 0).all()


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_cuts_cover_the_boundaries(name):
    c = FC.CASES[name]
    K, L, _ = _design(c)
    P, Q = FC.ratio(c)
    r = FC.plan_shape(K, L, P, Q)[0]
    n_in = FC.n_input(K, P, Q, r)
    lens, outs, at = FC.cuts_by_outputs(K, P, Q, r, n_in)
    assert sum(lens) == n_in and sum(outs) == R.complete(K, P, Q, n_in)
    assert [outs[i] for i in at] == [0, 1, r - 1, r, r + 1]      # every wanted number is hit exactly
    assert lens[-1] > 0 and outs[-1] >= 1
    if P >= Q:                                         # (an input sample completes one output at the most)
        assert at == [0, 1, 2, 3, 4] and len(lens) == 6
    else:                                              # (one-sample calls in between, a few)
        extra = [i for i in range(len(lens) - 1) if i not in at]
        assert all(lens[i] == 1 for i in extra) and len(extra) <= 12, (lens, outs, at)
    lens = FC.cuts_by_length(K, n_in)
    assert sum(lens) == n_in and lens[:2] == [0, K - 1] and lens.count(1) >= 40 and lens[-1] > 0


def test_bound_follows_its_formula():
    """bound() on an input of ones is (K + 16) 2^-24 times the row sums of max(|T[j]|, |T[j + 1]|)."""
    c = FC.CASES['odd']
    K, L, T = _design(c)
    P, Q = FC.ratio(c)
    n = 7
    I, rem = divmod(n * P, Q)
    j = rem * L // Q
    x = np.ones(I + K, dtype=np.complex128)
    b = FC.bound(x, K, L, T, P, Q, n, n + 1)
    A = np.maximum(np.abs(T[j].astype(np.float64)), np.abs(T[j + 1].astype(np.float64)))
    assert I - K // 2 + 1 >= 0
    np.testing.assert_allclose(b, [(K + 16) * 2.0 ** -24 * A.sum()], rtol=1e-13)
    # input before index 0 and past the end counts as zero
    b0 = FC.bound(x[:3], K, L, T, P, Q, 0, 1)
    m = np.arange(K)
    inside = (m - K // 2 + 1 >= 0) & (m - K // 2 + 1 < 3)
    A0 = np.maximum(np.abs(T[0].astype(np.float64)), np.abs(T[1].astype(np.float64)))
    np.testing.assert_allclose(b0, [(K + 16) * 2.0 ** -24 * A0[inside].sum()], rtol=1e-13)
