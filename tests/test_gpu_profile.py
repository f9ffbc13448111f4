"""GPU: the multi-tap correlation profiles (gpsmi_acq_profile / AcqEngine.profiles)
against the float64 restatement (profile_ref.py), their bit-for-bit properties, the equivalence of the
inputs and entry points, and what a call leaves of the handle.

Shapes: n = 6 * 2048 + 123 at 2048 with Lh = 1, 8 and 32, one block of 130944 at 16368 with Lh = 32 and
5, and -- runs of 20 windows do not fit those -- 45 * 2048 + 57 at 2048 for coh_ms = 20.  Records, all
in one call: both Doppler signs, code starts within a sample of 0 (the first windows fall away), just
below cs and negative, PRN 4 twice, a record whose last window ends flush with n, skip_ms 0 and 7 (1 on
the short inputs); with coh_ms = 3 the records hold one and two runs.

Tolerance against the restatement, per case and formed in the test: four times what a plain numpy
float32 evaluation of the same sums (profile_ref.prof_ref(plain32=True): the same quantised carrier,
numpy's own summation order) deviates from the float64 restatement, max |S - S_ref| / max |S_ref| and the
same for Q over its trace, under the hard cap of 1e-4.  The deviations the MI355X shows stand in
DESIGN.md 4.2r."""
import numpy as np
import pytest

import profile_ref as R
from test_gpu_acq_noncoherent import CFG, _same, _upload

pytestmark = pytest.mark.gpu

CAP = 1e-4
# (cs, input, Lh, coh_ms)
CASES = [(2048, 'short', 1, 1), (2048, 'short', 8, 3), (2048, 'short', 32, 1), (2048, 'long', 8, 20),
         (2048, 'long', 32, 3), (16368, 'short', 32, 3), (16368, 'short', 5, 1)]


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


def data_of(cs, which, raw):
    return R.kernel_raw(cs, which) if raw else R.kernel_c64(cs, which)


def on_device(e, x, sats, **kw):
    buf = _upload(x)
    try:
        return e.profiles((buf.ptr, len(x)), sats, **kw)
    finally:
        buf.free()


def bounds(cs, which, Lh, coh, n_runs=0):
    """(S_ref, Q_ref, n_ref, tol_s, tol_q): the restatement and four times the plain float32 deviation."""
    S_ref, Q_ref, n_ref = R.kernel_reference(cs, which, Lh, coh, n_runs)
    S_32, Q_32, _ = R.kernel_reference(cs, which, Lh, coh, n_runs, plain32=True)
    d_s, d_q = R.deviation(S_32, Q_32, S_ref, Q_ref)
    assert 0 < 4 * d_s <= CAP and 0 < 4 * d_q <= CAP
    return S_ref, Q_ref, n_ref, 4 * d_s, 4 * d_q


@pytest.mark.parametrize('cs,which,Lh,coh', CASES, ids=lambda v: str(v))
def test_against_the_restatement(engines, cs, which, Lh, coh):
    S_ref, Q_ref, n_ref, tol_s, tol_q = bounds(cs, which, Lh, coh)
    K = 2 * Lh + 1
    for raw in (False, True):
        e = engines(cs, raw)
        x = data_of(cs, which, raw)
        sats = R.kernel_records(cs, len(x), Lh)
        cov, n_runs, S = e.profiles(x, sats, half_taps=Lh, coh_ms=coh, sums=True)
        assert e.last_ms() > 0
        assert np.array_equal(n_runs, n_ref) and S.shape == S_ref.shape == (len(sats), K, n_ref.max())
        assert cov.shape == Q_ref.shape == (len(sats), K, K)
        if coh == 3:
            assert set(n_runs.tolist()) >= {1, 2} if which == 'short' else len(set(n_runs.tolist())) > 1
        for r, w in enumerate(n_runs):
            assert np.all(S[r, :, w:] == 0)                       # zero past a record's last run
        # bit for bit: the lower triangle is the conjugate of the upper, the diagonal is real
        assert np.array_equal(cov, np.conj(np.transpose(cov, (0, 2, 1))))
        assert np.all(np.diagonal(cov, axis1=1, axis2=2).imag == 0) and np.all(np.diagonal(cov, axis1=1, axis2=2).real > 0)
        d_s, d_q = R.deviation(S, cov, S_ref, Q_ref)
        print('deviations cs %d %s Lh %d coh %d raw %d: S %.3e (bound %.3e)  Q %.3e (bound %.3e)'
              % (cs, which, Lh, coh, raw, d_s, tol_s, d_q, tol_q))
        assert d_s <= tol_s and d_q <= tol_q
        # the covariance is the float64 sum of the sums that came back, to float64's rounding
        q_of_s = np.einsum('rlm,rkm->rlk', S.astype(np.complex128), S.astype(np.complex128).conj())
        np.testing.assert_allclose(cov, q_of_s, rtol=0, atol=1e-13 * np.abs(q_of_s).max())
        # the same bytes again, from device memory too, and raw = its complex64 decode
        for got in (e.profiles(x, sats, half_taps=Lh, coh_ms=coh, sums=True),
                    on_device(e, x, sats, half_taps=Lh, coh_ms=coh, sums=True)):
            _same(got[0], cov), _same(got[1], n_runs), _same(got[2], S)
        if raw:
            _same(cov, first[0]), _same(S, first[2])
        first = (cov, n_runs, S)


@pytest.mark.parametrize('cs,which,Lh,coh', [(2048, 'short', 8, 1), (2048, 'long', 32, 3), (16368, 'short', 32, 3)],
                         ids=lambda v: str(v))
def test_a_record_depends_on_itself_alone(engines, cs, which, Lh, coh):
    """A record alone, among others, in another place of the call and beside its own copy: the same
    bytes."""
    e = engines(cs, False)
    x = data_of(cs, which, False)
    sats = R.kernel_records(cs, len(x), Lh)
    kw = dict(half_taps=Lh, coh_ms=coh, sums=True)
    cov, n_runs, S = e.profiles(x, sats, **kw)
    for r, s in enumerate(sats):
        c1, n1, S1 = e.profiles(x, [s], **kw)
        assert n1[0] == n_runs[r]
        _same(c1[0], cov[r]), _same(S1[0], S[r][:, :n_runs[r]])
    order = [3, 1, 1, 4, 0, 2]
    c2, n2, S2 = e.profiles(x, [sats[i] for i in order], **kw)
    for k, i in enumerate(order):
        _same(c2[k], cov[i]), _same(S2[k], S[i])


def test_a_tap_does_not_depend_on_the_taps_around_it(engines):
    """The taps a smaller half_taps keeps are the larger one's, bit for bit, as far as the windows are
    the same ones (a record in mid-input: its windows do not move with Lh)."""
    e = engines(2048, False)
    x = data_of(2048, 'short', False)
    sat = [(9, 0, 402.0, 1347.4)]
    big = e.profiles(x, sat, half_taps=32, coh_ms=1, sums=True)
    for Lh in (1, 8, 9):
        small = e.profiles(x, sat, half_taps=Lh, coh_ms=1, sums=True)
        assert small[1][0] == big[1][0]
        _same(small[2][0], big[2][0][32 - Lh:32 + Lh + 1])
        _same(small[0][0], big[0][0][32 - Lh:32 + Lh + 1, 32 - Lh:32 + Lh + 1])


def test_n_runs_and_skip(engines):
    e = engines(2048, False)
    x = data_of(2048, 'long', False)
    sats = R.kernel_records(2048, len(x), 8)
    cov, n_runs, S = e.profiles(x, sats, half_taps=8, coh_ms=3, sums=True)
    assert n_runs.min() >= 12
    c2, n2, S2 = e.profiles(x, sats, half_taps=8, coh_ms=3, n_runs=2, sums=True)
    assert n2.tolist() == [2] * len(sats) and S2.shape[2] == 2
    _same(S2, S[:, :, :2])
    _, Q_ref, _, _, tol_q = bounds(2048, 'long', 8, 3, 2)
    assert R.deviation(S2, c2, S2, Q_ref)[1] <= tol_q
    c9, n9 = e.profiles(x, sats, half_taps=8, coh_ms=3, n_runs=99)         # more than fit: all of them
    _same(c9, cov), _same(n9, n_runs)
    # skip_ms moves the runs along the windows: skip 3 at coh_ms 3 is run 1 of skip 0
    prn, _, f, tau = sats[2]
    a = e.profiles(x, [(prn, 0, f, tau)], half_taps=8, coh_ms=3, sums=True)
    b = e.profiles(x, [(prn, 3, f, tau)], half_taps=8, coh_ms=3, sums=True)
    assert b[1][0] == a[1][0] - 1
    _same(b[2][0], a[2][0][:, 1:])
    # the defaults: 8 taps either side, 20-ms runs
    d = e.profiles(x, sats, sums=True)
    _same(d[2], e.profiles(x, sats, half_taps=8, coh_ms=20, sums=True)[2])


@pytest.mark.parametrize('cs', [2048, 16368])
def test_centre_tap_is_the_signature_prompt(engines, cs):
    """Tap l = 0 with coh_ms = 1 against gpsmi_acq_signature's prompt of the same record and window:
    two float32 evaluations of one sum, within the case's tolerance (four times the plain float32
    deviation from the restatement, over max |S_ref|)."""
    import sig_ref
    e = engines(cs, False)
    x = data_of(cs, 'short', False)
    Lh = 8
    sats = [(p, 0, f, tau) for p, _, f, tau in R.kernel_records(cs, len(x), Lh)]
    S_ref, _, _, tol_s, _ = bounds(cs, 'short', Lh, 1)
    cov, n_runs, S = e.profiles(x, sats, half_taps=Lh, coh_ms=1, sums=True)
    _, n_win, P = e.signatures(np.stack([x, x]), [(p, f, tau) for p, _, f, tau in sats], 2, prompts=True)
    scale = np.abs(S_ref).max()
    seen = 0
    for r, (p, _, f, tau) in enumerate(sats):
        js = sig_ref.sig_windows(len(x), cs, f, tau)
        jp = R.prof_windows(len(x), cs, f, tau, Lh, 0, 1)[:, 0]
        assert len(js) == n_win[r] and len(jp) == n_runs[r]
        for m, j in enumerate(jp):
            dev = abs(complex(S[r, Lh, m]) - complex(P[r, 0, js.index(int(j))])) / scale
            assert dev <= tol_s, (r, m, dev)
            seen += 1
    assert seen >= 20


def test_other_calls_and_refusals_leave_the_handle_as_it_was():
    """gpsmi_acq_signature and gpsmi_acq_refine before and after profiles on one handle: the same
    bytes; what needs the handle to be refused -- a PRN without a replica, a null pointer -- and the
    plan's refusals leave it usable."""
    import ctypes as C

    from gpsmi import _lib
    from gpsmi.engine import AcqEngine, Config, EngineError
    e = AcqEngine(Config(**CFG[2048]))
    x = data_of(2048, 'long', False)
    n = len(x)
    sats = R.kernel_records(2048, n, 8)
    sig_sats = [(p, f, tau) for p, _, f, tau in sats]
    hits = [(4, 3100.0, 0), (9, 400.0, 1347)]
    try:
        sig0 = e.signatures(np.stack([x, x]), sig_sats, 2, prompts=True)
        ref0 = e.refine(x, hits, 40)
        cov, n_runs, S = e.profiles(x, sats, sums=True)
        for a, b in zip(e.signatures(np.stack([x, x]), sig_sats, 2, prompts=True), sig0):
            _same(a, b)
        _same(e.refine(x, hits, 40), ref0)
        sat = np.zeros(1, _lib.PROF_SAT_DTYPE)
        sat[0] = (17, 0, 100.0, 3.0)
        K = 17
        c, w = np.zeros((1, K, K), np.complex128), np.zeros(1, np.int32)
        cfg = _lib.ProfCfg(0, 0, 0, 0, 0.0, 0.0)
        rc = e.lib.gpsmi_acq_profile(e.h, _lib.ptr(x), n, _lib.ptr(sat), 1, C.byref(cfg), _lib.ptr(c), _lib.ptr(w), None)
        assert rc == -3 and 'PRN 17' in e.lib.gpsmi_last_error().decode()
        rc = e.lib.gpsmi_acq_profile(e.h, _lib.ptr(x), n, _lib.ptr(sat), 1, C.byref(cfg), None, _lib.ptr(w), None)
        assert rc == -1 and 'null' in e.lib.gpsmi_last_error().decode()
        for bad in ([(4, 0, np.nan, 0.0)], [(4, 0, 0.0, np.inf)], [(40, 0, 0.0, 0.0)], [(4, 20, 0.0, 0.0)], []):
            with pytest.raises(EngineError):
                e.profiles(x, bad)
        with pytest.raises(EngineError):
            e.profiles(x[:20 * 2048], sats)                       # no run of 20 windows fits
        with pytest.raises(ValueError):
            e.profiles(np.stack([x, x]), sats)                    # one antenna
        got = e.profiles(x, sats, sums=True)
        _same(got[0], cov), _same(got[1], n_runs), _same(got[2], S)
        for a, b in zip(e.signatures(np.stack([x, x]), sig_sats, 2, prompts=True), sig0):
            _same(a, b)
        _same(e.refine(x, hits, 40), ref0)
    finally:
        e.close()
