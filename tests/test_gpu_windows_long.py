"""GPU: cancellation, signatures and profiles against their float64
restatements on the calls of windows_cases.py -- window starts that slip by a sample, windows of 1.01 cs,
f_offset_hz and carrier_hz that reach the kernels, a carrier at 0.44 fs, 300 and 257 windows to a record,
records a window apart in one call, heads of the same rows, samples two million in -- and the bit-for-bit
properties that hold across them.  test_windows_cases.py (CPU) holds that the calls are what they are
called.

Bounds: none of this module's own.  Signatures and cancellation are held to test_gpu_signature.TOL and
test_gpu_cancel.TOL / ENERGY_RTOL, profiles to four times the deviation of the plain float32 restatement
of the same call (profile_ref.prof_ref(plain32=True)) under test_gpu_profile.CAP, as test_gpu_profile
forms it: a window's sum has the terms it has there (at most 1.011 times as many in cancellation) and
a covariance is measured over its own trace, so neither more windows nor later ones are a reason for
more.  Every comparison prints `windows_long <stage> <call> <metric> measured / bound`; the figures
of the MI355X stand in DESIGN.md 4.2j, 4.2p and 4.2r."""
import numpy as np
import pytest

import profile_ref as PR
import test_gpu_cancel as TC
import test_gpu_profile as TP
import test_gpu_signature as TS
import windows_cases as W
from test_gpu_acq_noncoherent import CFG, _same, _upload

pytestmark = pytest.mark.gpu

SLIPS = [W.slip(nm, cs) for cs in (2048, 16368) for nm in W.SLIP_NAMES]
MANY = {cs: [W.many_at(cs, n) for n in W.MANY_N[cs]] for cs in (2048, 16368)}
STALE = W.many_at(2048, W.STALE_N)
LATE = W.late()
# (call, antennas, n_ms)
SIG_CASES = [(c, 2, 0) for c in SLIPS] + [(c, A, 0) for c in MANY[2048] for A in (2, 8)] + \
            [(c, 4, 0) for c in MANY[16368]] + [(LATE, 2, 0), (LATE, 2, 3)]
PROF_CASES = [(c, p) for c in SLIPS + [MANY[2048][0], MANY[16368][0], LATE] for p in W.prof_settings(c)]
CANCEL_CASES = [(c, False) for c in SLIPS] + [(LATE, True)]


def case_id(v):
    return v.id if isinstance(v, W.Call) else '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope='module')
def engines():
    from gpsmi.engine import AcqEngine, Config
    made = {}

    def get(cs, raw):
        if (cs, raw) not in made:
            e = AcqEngine(Config(**CFG[cs]))
            e.set_input_format(raw)
            made[cs, raw] = e
        return made[cs, raw]
    yield get
    for e in made.values():
        e.close()


def fresh(cs):
    from gpsmi.engine import AcqEngine, Config
    return AcqEngine(Config(**CFG[cs]))


def report(stage, call, what, measured, bound):
    print('windows_long %-9s %-20s %-6s %.3e / %.3e = %.2f' % (stage, call.id, what, measured, bound, measured / bound))


# ---- the three stages as the tests call them ----------------------------------------------------
def signatures(e, call, A, raw=False, dev=False, **kw):
    x = W.rows(call, A, raw)
    buf = _upload(x) if dev else None
    try:
        return e.signatures((buf.ptr, call.n) if dev else x, list(call.records), A, prompts=True, **call.opts, **kw)
    finally:
        if buf is not None:
            buf.free()


def profiles(e, call, p, raw=False, dev=False, **kw):
    x = W.rows(call, 0, raw)
    buf = _upload(x) if dev else None
    try:
        return e.profiles((buf.ptr, call.n) if dev else x, call.prof_records(p.skip), sums=True,
                          **{**p.kw, **kw}, **call.opts)
    finally:
        if buf is not None:
            buf.free()


def cancel(e, call, raw=False, dev=False):
    from gpsmi.engine import DeviceBuffer
    x = W.rows(call, 0, raw)
    if not dev:
        return e.cancel(x, list(call.records), coef=True, **call.opts)
    d_in, d_out = _upload(x), DeviceBuffer(8 * call.n)
    try:
        _, rec, coef = e.cancel((d_in.ptr, call.n), list(call.records), out=d_out.ptr, coef=True, **call.opts)
        return d_out.download(np.complex64, call.n), rec, coef
    finally:
        d_in.free(), d_out.free()


# ---- what a result is held to -------------------------------------------------------------------
def hermitian(cov):
    """By value: the lower triangle is the conjugate of the upper, the diagonal real and positive."""
    assert np.array_equal(cov, np.conj(np.transpose(cov, (0, 2, 1))))
    d = np.diagonal(cov, axis1=1, axis2=2)
    assert np.all(d.imag == 0) and np.all(d.real > 0)


def is_sum_of(cov, sums):
    """cov is the float64 sum over the prompts or sums that came back, to float64's rounding."""
    s = sums.astype(np.complex128)
    want = np.einsum('rak,rbk->rab', s, s.conj())
    np.testing.assert_allclose(cov, want, rtol=0, atol=1e-13 * np.abs(want).max())


def check_signatures(call, A, n_ms, got, label='sig'):
    cov, n_win, P = got
    P_ref, C_ref, n_ref = W.sig_reference(call, A, n_ms)
    assert np.array_equal(n_win, n_ref) and P.shape == P_ref.shape and cov.shape == C_ref.shape
    for r, w in enumerate(n_win):
        assert np.all(P[r, :, w:] == 0)
    hermitian(cov)
    d_p = np.abs(P - P_ref).max() / np.abs(P_ref).max()
    d_c = max(np.abs(cov[r] - C_ref[r]).max() / np.trace(C_ref[r]).real for r in range(len(n_ref)))
    tol = TS.TOL[call.cs]
    assert max(tol.values()) <= TS.CAP
    report(label, call, 'A%d' % A + ('n%d' % n_ms if n_ms else '') + ' P', d_p, tol['prompt'])
    report(label, call, 'A%d' % A + ('n%d' % n_ms if n_ms else '') + ' C', d_c, tol['cov'])
    assert d_p <= tol['prompt'] and d_c <= tol['cov']
    is_sum_of(cov, P)


def prof_bounds(call, p):
    """(S_ref, Q_ref, n_ref, tol_s, tol_q): the restatement and four times the plain float32 deviation."""
    args = (call, p.Lh, p.coh, p.n_runs, p.skip)
    S_ref, Q_ref, n_ref = W.prof_reference(*args)
    S_32, Q_32, _ = W.prof_reference(*args, plain32=True)
    d_s, d_q = PR.deviation(S_32, Q_32, S_ref, Q_ref)
    assert 0 < 4 * d_s <= TP.CAP and 0 < 4 * d_q <= TP.CAP
    return S_ref, Q_ref, n_ref, 4 * d_s, 4 * d_q


def check_profiles(call, p, got, label='prof'):
    cov, n_runs, S = got
    S_ref, Q_ref, n_ref, tol_s, tol_q = prof_bounds(call, p)
    K = 2 * p.Lh + 1
    assert np.array_equal(n_runs, n_ref) and S.shape == S_ref.shape == (len(n_ref), K, n_ref.max())
    assert cov.shape == Q_ref.shape
    for r, w in enumerate(n_runs):
        assert np.all(S[r, :, w:] == 0)
    hermitian(cov)
    d_s, d_q = PR.deviation(S, cov, S_ref, Q_ref)
    what = 'L%dc%d' % (p.Lh, p.coh) + ('s%d' % p.skip if p.skip else '') + ('r%d' % p.n_runs if p.n_runs else '')
    report(label, call, what + ' S', d_s, tol_s)
    report(label, call, what + ' Q', d_q, tol_q)
    assert d_s <= tol_s and d_q <= tol_q
    is_sum_of(cov, S)


def check_cancel(call, got, label='cancel'):
    y, rec, coef = got
    y_ref, rec_ref, coef_ref, done = W.cancel_reference(call)
    x0 = W.c64(call)[0]
    assert rec['prn'].tolist() == [s[0] for s in call.records]
    assert np.array_equal(rec['n_windows'], rec_ref['n_windows']) and np.array_equal(rec['n_skipped'], rec_ref['n_skipped'])
    assert rec['n_windows'].tolist() == [len(w) for w in W.cancel_wins(call)]
    np.testing.assert_allclose(rec['energy_in'], rec_ref['energy_in'], rtol=TC.ENERGY_RTOL)
    np.testing.assert_allclose(rec['energy_removed'], rec_ref['energy_removed'], rtol=TC.ENERGY_RTOL)
    assert coef.shape == coef_ref.shape and np.all(coef[coef_ref == 0] == 0)
    # a skipped window leaves its samples bit for bit (and so does what no processed window holds)
    untouched = ~done.any(axis=0)
    _same(y[untouched], x0[untouched])
    rms = np.sqrt(np.mean(np.abs(x0.astype(np.complex128)) ** 2))
    d_out = np.abs(y - y_ref).max() / rms
    d_coef = np.abs(coef - coef_ref).max() / np.abs(coef_ref).max()
    tol = TC.TOL[call.cs]
    assert max(tol.values()) <= TC.CAP
    report(label, call, 'out', d_out, tol['out'])
    report(label, call, 'coef', d_coef, tol['coef'])
    assert d_out <= tol['out'] and d_coef <= tol['coef']
    return untouched


# ---- against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize('call,A,n_ms', SIG_CASES, ids=case_id)
def test_signatures_against_the_restatement(engines, call, A, n_ms):
    check_signatures(call, A, n_ms, signatures(engines(call.cs, False), call, A, n_ms=n_ms))


@pytest.mark.parametrize('call,p', PROF_CASES, ids=case_id)
def test_profiles_against_the_restatement(engines, call, p):
    check_profiles(call, p, profiles(engines(call.cs, False), call, p))


@pytest.mark.parametrize('call,raw', CANCEL_CASES, ids=case_id)
def test_cancellation_against_the_restatement(engines, call, raw):
    untouched = check_cancel(call, cancel(engines(call.cs, raw), call, raw))
    skipped = W.cancel_reference(call)[1]['n_skipped'].tolist()
    if call.name == 'fast':                           # its first window, one sample, is skipped
        assert skipped == [1] and untouched.sum() == 1 and untouched[0]
    elif call.name == 'natural' and call.cs == 2048:  # [0, 16) is min_window long: processed
        assert skipped == [0, 0] and not untouched.any()
    if call is LATE:
        assert W.cancel_reference(call)[1]['n_windows'].tolist() == [1006, 1005]


# ---- exact: fewer windows of the same call ------------------------------------------------------
def test_n_ms_takes_the_first_windows(engines):
    e, call = engines(2048, False), MANY[2048][0]
    cov, n_win, P = signatures(e, call, 2)
    assert n_win.tolist() == W.MANY_WINDOWS[2048][0]
    for n_ms in (8, 9, 17, 256, 257):
        c, n, Pn = signatures(e, call, 2, n_ms=n_ms)
        assert n.tolist() == [n_ms] * 3 and Pn.shape[2] == n_ms
        _same(Pn, P[:, :, :n_ms])
        hermitian(c), is_sum_of(c, Pn)


def test_n_runs_takes_the_first_runs(engines):
    e, call = engines(2048, False), MANY[2048][0]
    for p in (W.Prof(8, 1), W.Prof(32, 1)):
        cov, n_runs, S = profiles(e, call, p)
        assert n_runs.tolist() == [299] * 3
        for k in (1, 2, 299):
            c, n, Sk = profiles(e, call, p, n_runs=k)
            assert n.tolist() == [k] * 3 and Sk.shape[2] == k
            _same(Sk, S[:, :, :k])
            hermitian(c), is_sum_of(c, Sk)
            if k == 299:
                _same(c, cov)


@pytest.mark.parametrize('cs', [2048, 16368])
def test_a_head_of_the_rows_gives_the_same_bytes(engines, cs):
    """The same absolute indices, another max_windows (max_runs): the windows that fit the head are the
    whole call's, bit for bit."""
    e = engines(cs, False)
    A = 2 if cs == 2048 else 4
    whole, heads = MANY[cs][0], MANY[cs][1:] + ([STALE] if cs == 2048 else [])
    _, n_win, P = signatures(e, whole, A)
    p = W.prof_settings(whole)[0]
    _, n_runs, S = profiles(e, whole, p)
    for head in heads:
        _, n_h, P_h = signatures(e, head, A)
        assert P_h.shape[2] == n_h.max() < n_win.min()
        _, r_h, S_h = profiles(e, head, p)
        assert S_h.shape[2] == r_h.max() < n_runs.min()
        for r in range(3):
            _same(P_h[r][:, :n_h[r]], P[r][:, :n_h[r]])
            _same(S_h[r][:, :r_h[r]], S[r][:, :r_h[r]])


def test_a_smaller_call_sees_nothing_of_the_one_before(engines):
    """Straight after the 300-window call, on the same handle, 19, 18 and 18 windows: zero past each
    record's count, and the bytes of a handle that never held anything."""
    e = engines(2048, False)
    new = fresh(2048)
    try:
        signatures(e, MANY[2048][0], 8)
        cov, n_win, P = signatures(e, STALE, 2)
        assert n_win.tolist() == [19, 18, 18] and np.all(P[1:, :, 18] == 0) and np.all(P[0, :, 18] != 0)
        for a, b in zip((cov, n_win, P), signatures(new, STALE, 2)):
            _same(a, b)
        check_signatures(STALE, 2, 0, (cov, n_win, P), 'sig-after')
        p = W.Prof(8, 1)
        profiles(e, MANY[2048][0], W.Prof(32, 1))
        other = STALE.on_the_same_rows(STALE.records[:1] + ((5, -4319.0, 20.3), STALE.records[2]))
        for call, runs in ((STALE, [18, 18, 18]), (other, [18, 19, 18])):
            cov, n_runs, S = profiles(e, call, p)
            assert n_runs.tolist() == runs
            for r, w in enumerate(n_runs):
                assert np.all(S[r, :, w:] == 0) and np.all(S[r, :, :w] != 0)
            for a, b in zip((cov, n_runs, S), profiles(new, call, p)):
                _same(a, b)
        check_profiles(STALE, p, profiles(e, STALE, p), 'prof-after')
    finally:
        new.close()


# ---- exact: entry points; formats within the bound ----------------------------------------------
@pytest.mark.parametrize('call,A', [(W.slip('slow', 2048), 2), (W.slip('slow', 16368), 2), (MANY[2048][0], 8)], ids=case_id)
def test_entry_points_and_formats(engines, call, A):
    """Host and device memory: the same bytes; raw and complex64 input: both within the bound of the
    restatement (which is of the decoded raw samples)."""
    p = W.prof_settings(call)[0]
    for raw in (False, True):
        e = engines(call.cs, raw)
        tag = 'u8' if raw else 'c64'
        host = signatures(e, call, A, raw)
        for a, b in zip(host, signatures(e, call, A, raw, dev=True)):
            _same(a, b)
        check_signatures(call, A, 0, host, 'sig-' + tag)
        if call.name != 'slow':
            continue
        host = profiles(e, call, p, raw)
        for a, b in zip(host, profiles(e, call, p, raw, dev=True)):
            _same(a, b)
        check_profiles(call, p, host, 'prof-' + tag)
        host = cancel(e, call, raw)
        for a, b in zip(host, cancel(e, call, raw, dev=True)):
            _same(a, b)
        check_cancel(call, host, 'cancel-' + tag)


# ---- two kernels, one sum -----------------------------------------------------------------------
@pytest.mark.parametrize('call', [W.slip(nm, cs) for cs in (2048, 16368) for nm in ('slow', 'fast')], ids=case_id)
def test_centre_tap_is_the_signature_prompt(engines, call):
    """Tap l = 0 with coh_ms = 1 against the signature's prompt of the same record and window, as
    test_gpu_profile.test_centre_tap_is_the_signature_prompt holds them: two float32 evaluations of one
    sum, within four times the plain float32 deviation from the restatement, over max |S_ref|."""
    e = engines(call.cs, False)
    p = W.Prof(8, 1)
    S_ref, _, _, tol_s, _ = prof_bounds(call, p)
    _, n_runs, S = profiles(e, call, p)
    _, n_win, P = signatures(e, call, 2)
    scale = np.abs(S_ref).max()
    seen, worst = 0, 0.0
    for r, (js, jp) in enumerate(zip(W.sig_starts(call), W.prof_starts(call, p.Lh, 1))):
        assert len(js) == n_win[r] and len(jp) == n_runs[r]
        for m, j in enumerate(jp[:, 0]):
            dev = abs(complex(S[r, p.Lh, m]) - complex(P[r, 0, js.index(int(j))])) / scale
            worst = max(worst, dev)
            assert dev <= tol_s, (r, m, dev)
            seen += 1
    report('tap0', call, 'L8c1', worst, tol_s)
    assert seen >= 18
