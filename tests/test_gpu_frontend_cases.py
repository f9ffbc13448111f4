"""The front-end kernels (csrc/gpsmi_fe.hip) on the pinned cases of tests/fe_cases.py: every output
against the float64 restatement (tests/fe_ref.py) within the derived bound of fe_cases.bound, single
taps on unit impulses, and the same bytes however the input is cut into calls, in every class of the
planner (workgroups of 256, 128, 64 outputs; dynamic LDS above 64 KiB)."""
import numpy as np
import pytest

import fe_cases as FC
import fe_ref as R

pytestmark = pytest.mark.gpu

MAX_OUT = 2048
_CACHE = {}


def _fe(c, **kw):
    from gpsmi.engine import Config
    from gpsmi.frontend import FrontEnd
    c = dict(c, **kw)
    fe = FrontEnd(Config(code_samples=c['fs_out'] // 1000), c['fs_in'], c['fmt'], c['if_hz'], c['conjugate'],
                  c['passband_hz'], c['atten_db'], max_out=MAX_OUT)
    return fe


def _case(name):
    """Design, class, noise input and float64 reference of a case (memoised; left unchanged)."""
    if name not in _CACHE:
        from gpsmi import frontend
        c = FC.CASES[name]
        K, L, T = frontend.design(c['fs_in'], c['fs_out'], c['fmt'], c['if_hz'], c['conjugate'], c['passband_hz'],
                                  c['atten_db'])
        P, Q = FC.ratio(c)
        r, lds = FC.plan_shape(K, L, P, Q)
        assert r == c['R'] and (lds > FC.LDS_BUDGET) == c['lds_hi']
        x = FC.noise_input(name, K, r)
        n_in = FC.samples(c, x)
        n_done, n_all = R.complete(K, P, Q, n_in), -(-n_in * Q // P)
        assert n_done >= 3 * r + 5 and n_all <= MAX_OUT
        xm = R.mix(R.decode(x, c['fmt']), c['if_hz'], c['fs_in'], 0, c['conjugate'])
        ref = R.resample(xm, K, L, T, P, Q, 0, n_all)
        B = FC.bound(xm, K, L, T, P, Q, 0, n_all)
        _CACHE[name] = dict(c=c, K=K, L=L, T=T, P=P, Q=Q, R=r, x=x, n_in=n_in, n_done=n_done, n_all=n_all,
                            ref=ref, B=B)
    return _CACHE[name]


def _single(name):
    """(outputs of one push of the noise input, outputs of the flush) on a handle of its own."""
    key = ('single', name)
    if key not in _CACHE:
        s = _case(name)
        fe = _fe(s['c'])
        assert fe.max_in >= s['n_in']                   # (one push is one call)
        assert (fe.n_taps, fe.n_phases) == (s['K'], s['L'])
        y = fe.push(s['x'])
        tail = fe.flush()
        fe.close()
        _CACHE[key] = (y, tail)
    return _CACHE[key]


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_noise_within_the_derived_bound(name):
    s = _case(name)
    y, tail = _single(name)
    assert len(y) == s['n_done'] and len(y) + len(tail) == s['n_all']
    got = np.concatenate([y, tail]).astype(np.complex128)
    err = np.abs(got - s['ref'])
    assert (s['B'] > 0).all()
    ratio = err / s['B']
    print(f'{name}: max |y - ref| / B = {ratio[:len(y)].max():.4f} (push), {ratio[len(y):].max():.4f} (flush); '
          f'max |y - ref| = {err.max():.3e}, rms ref = {np.sqrt(np.mean(np.abs(s["ref"]) ** 2)):.3e}')
    worst = int(ratio.argmax())
    assert (err <= s['B']).all(), (name, worst, err[worst], s['B'][worst])


def _check_impulse(s, i0, y):
    want, hit = FC.impulse_expected(s['K'], s['L'], s['T'], s['P'], s['Q'], i0, len(y))
    assert hit.any() and not hit.all()
    tol = 2.0 ** -21 * float(np.abs(s['T']).max())
    err = np.abs(y.astype(np.complex128) - want)
    assert err.max() <= tol, (i0, int(err.argmax()), err.max(), tol)
    assert (y[~hit] == 0).all(), (i0, np.flatnonzero(y[~hit] != 0)[:8])
    return err.max() / tol


@pytest.mark.parametrize('name', FC.IMPULSE_CASES)
def test_unit_impulse_reads_single_taps(name):
    s = _case(name)
    fe = _fe(s['c'])
    worst = 0.0
    for i0 in FC.impulse_positions(s['K'], s['P'], s['Q'], s['R']):
        x = np.zeros(s['n_in'], dtype=np.complex64)
        x[i0] = 1.0
        fe.reset()
        y = fe.push(x)
        assert len(y) == s['n_done']
        worst = max(worst, _check_impulse(s, i0, y))
        # the impulse as the last sample of a call: every output that sees it reads it from the carry
        fe.reset()
        before = fe.push(x[:i0 + 1])
        after = fe.push(x[i0 + 1:])
        assert len(after) > 0
        y2 = np.concatenate([before, after])
        assert len(y2) == s['n_done']
        worst = max(worst, _check_impulse(s, i0, y2))
        assert y2.tobytes() == y.tobytes()
    fe.close()
    print(f'{name}: max |y - expected| / (2^-21 max |T|) = {worst:.4f}')


def _push_cut(fe, c, x, lens):
    parts, pos = [], 0
    for m in lens:
        parts.append(fe.push(FC.cut(c, x, pos, pos + m)))
        pos += m
    assert pos == FC.samples(c, x)
    return parts


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_cuts_do_not_change_the_bytes(name):
    s = _case(name)
    c, x = s['c'], s['x']
    one, tail = _single(name)
    fe = _fe(c)
    lens, outs, at = FC.cuts_by_outputs(s['K'], s['P'], s['Q'], s['R'], s['n_in'])
    parts = _push_cut(fe, c, x, lens)
    assert [len(p) for p in parts] == outs
    assert [len(parts[i]) for i in at] == [0, 1, s['R'] - 1, s['R'], s['R'] + 1]
    assert np.concatenate(parts).tobytes() == one.tobytes()
    assert fe.flush().tobytes() == tail.tobytes()
    fe.reset()
    parts = _push_cut(fe, c, x, FC.cuts_by_length(s['K'], s['n_in']))
    assert len(parts[0]) == 0
    assert np.concatenate(parts).tobytes() == one.tobytes()
    assert fe.flush().tobytes() == tail.tobytes()
    fe.close()


def test_large_lds_handle_between_small_ones():
    """The dynamic-LDS limit of the filter kernel is raised per process, not per handle: handles of
    either kind, made and used in any order, give what they give alone."""
    lo, hi = _case('lo'), _case('lds_hi')
    want_lo, want_hi = _single('lo'), _single('lds_hi')
    fe_a = _fe(lo['c'])
    got_a = (fe_a.push(lo['x']), fe_a.flush())
    fe_hi = _fe(hi['c'])
    got_hi = (fe_hi.push(hi['x']), fe_hi.flush())
    fe_b = _fe(lo['c'])
    got_b = (fe_b.push(lo['x']), fe_b.flush())
    fe_a.reset()                                        # the handle made before the large one, used after it
    got_a2 = (fe_a.push(lo['x']), fe_a.flush())
    for got, want in ((got_a, want_lo), (got_hi, want_hi), (got_b, want_lo), (got_a2, want_lo)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    for fe in (fe_a, fe_hi, fe_b):
        fe.close()


def test_two_large_lds_handles_the_larger_made_first_and_used_last():
    """Two live handles above 64 KiB of different sizes: making the smaller one (76 568 B) must not take
    from the larger one (91 576 B) the dynamic LDS its next launch asks for."""
    big, small = _case('lds_hi60'), _case('lds_hi')
    want_big, want_small = _single('lds_hi60'), _single('lds_hi')
    assert FC.plan_shape(big['K'], big['L'], big['P'], big['Q'])[1] > \
        FC.plan_shape(small['K'], small['L'], small['P'], small['Q'])[1] > FC.LDS_BUDGET
    fe_big = _fe(big['c'])
    fe_small = _fe(small['c'])
    got_small = (fe_small.push(small['x']), fe_small.flush())
    got_big = (fe_big.push(big['x']), fe_big.flush())
    for got, want in ((got_small, want_small), (got_big, want_big)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    fe_big.close()
    fe_small.close()


def test_if_beyond_fs_in_wraps():
    s = _case('wrap')
    y, tail = _single('wrap')
    fe = _fe(s['c'], if_hz=312_500.0)
    assert fe.push(s['x']).tobytes() == y.tobytes()
    assert fe.flush().tobytes() == tail.tobytes()
    fe.close()
