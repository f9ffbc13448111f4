"""GPU: the spatial signatures (gpsmi_acq_signature / AcqEngine.signatures) against
the float64 restatement (sig_ref.py), their bit-for-bit properties, the equivalence of the inputs and
entry points, and what a call leaves of the handle.

Shapes: n = 6 * 2048 + 123 at 2048 with 2, 3 and 8 antennas, one block of 130944 at 16368 with 2 and 4.
Records, all in one call: both Doppler signs, code starts within a sample of 0, just below cs and
negative, and PRN 4 twice at two code starts.

Tolerances against the restatement: the GPU sums the prompts in float32 and takes its carrier from 24
bits of an integer phase, so the deviations were measured on the first GPU run (MI355X, the largest
over all cases of a code length) and are asserted at four times that, under the hard cap of 1e-4;
the measured values stand beside each constant and in DESIGN.md 4.2p."""
import numpy as np
import pytest

import sig_ref as R
from test_gpu_acq_noncoherent import CFG, _same, _upload

pytestmark = pytest.mark.gpu

CAP = 1e-4
# asserted = 4 x the largest deviation measured on the first GPU run           measured
TOL = {2048: dict(prompt=4 * 2.533e-07,      # max |P - P_ref| / max |P_ref|     2.533e-07 (every A, both formats)
                  cov=4 * 2.669e-08),        # max |C - C_ref| / trace(C_ref)    2.669e-08 (A = 2)
       16368: dict(prompt=4 * 2.435e-07,     #                                   2.435e-07 (every A, both formats)
                   cov=4 * 3.632e-08)}       #                                   3.632e-08 (A = 2)
assert all(v <= CAP for t in TOL.values() for v in t.values())

MEASURED = {2048: dict(prompt=0.0, cov=0.0), 16368: dict(prompt=0.0, cov=0.0)}
SHAPES = [(cs, A, raw) for cs in (2048, 16368) for A in R.KERNEL_ANTENNAS[cs] for raw in (False, True)]


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


def rows_of(cs, A, raw):
    return np.ascontiguousarray((R.kernel_raw(cs) if raw else R.kernel_c64(cs))[:A])


def on_device(e, rows, sats, **kw):
    buf = _upload(rows)
    try:
        return e.signatures((buf.ptr, rows.shape[1]), sats, rows.shape[0], **kw)
    finally:
        buf.free()


@pytest.mark.parametrize('cs,A,raw', SHAPES, ids=lambda v: str(v))
def test_against_the_restatement(engines, cs, A, raw):
    e = engines(cs, raw)
    sats = R.kernel_records(cs)
    P_ref, C_ref, n_ref = R.kernel_reference(cs, A)
    cov, n_win, P = e.signatures(rows_of(cs, A, raw), sats, A, prompts=True)
    assert e.last_ms() > 0
    assert np.array_equal(n_win, n_ref) and P.shape == P_ref.shape and cov.shape == C_ref.shape
    assert n_win.tolist() == ([6, 6, 5, 5] if cs == 2048 else [8, 8, 7, 7])
    for r, w in enumerate(n_win):
        assert np.all(P[r, :, w:] == 0)                       # zero past a record's last window
    # bit for bit: the lower triangle is the conjugate of the upper, the diagonal is real
    # (values, not bytes: the conjugate of the diagonal's +0 is -0)
    assert np.array_equal(cov, np.conj(np.transpose(cov, (0, 2, 1))))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2).imag == 0) and np.all(np.diagonal(cov, axis1=1, axis2=2).real > 0)
    # the numbers
    d_p = np.abs(P - P_ref).max() / np.abs(P_ref).max()
    d_c = max(np.abs(cov[r] - C_ref[r]).max() / np.trace(C_ref[r]).real for r in range(len(sats)))
    print('deviations cs %d A %d raw %d: prompt %.3e  cov %.3e' % (cs, A, raw, d_p, d_c))
    MEASURED[cs]['prompt'] = max(MEASURED[cs]['prompt'], d_p)
    MEASURED[cs]['cov'] = max(MEASURED[cs]['cov'], d_c)
    print('largest so far cs %d: prompt %.3e  cov %.3e' % (cs, MEASURED[cs]['prompt'], MEASURED[cs]['cov']))
    assert d_p <= TOL[cs]['prompt'] and d_c <= TOL[cs]['cov']
    # the covariance is the float64 sum of the prompts that came back, to float64's rounding
    c_of_p = np.einsum('rak,rbk->rab', P.astype(np.complex128), P.astype(np.complex128).conj())
    np.testing.assert_allclose(cov, c_of_p, rtol=0, atol=1e-13 * np.abs(c_of_p).max())
    # the same bytes again
    cov2, n2, P2 = e.signatures(rows_of(cs, A, raw), sats, A, prompts=True)
    _same(cov, cov2), _same(n_win, n2), _same(P, P2)


@pytest.mark.parametrize('cs,A', [(2048, 3), (2048, 8), (16368, 4)])
def test_entry_points_and_formats_agree(engines, cs, A):
    """Host and device memory, raw and complex64 input: one result."""
    sats = R.kernel_records(cs)
    res = engines(cs, False).signatures(rows_of(cs, A, False), sats, A, prompts=True)
    for raw in (False, True):
        e = engines(cs, raw)
        for got in (e.signatures(rows_of(cs, A, raw), sats, A, prompts=True),
                    on_device(e, rows_of(cs, A, raw), sats, prompts=True)):
            for a, b in zip(got, res):
                _same(a, b)


@pytest.mark.parametrize('cs', [2048, 16368])
def test_a_record_depends_on_itself_alone(engines, cs):
    """A record alone, among others, in another place of the call and beside its own copy: the same
    bytes; fewer antennas: the same bytes for the antennas that stay."""
    e = engines(cs, False)
    sats = R.kernel_records(cs)
    A = max(R.KERNEL_ANTENNAS[cs])
    rows = rows_of(cs, A, False)
    cov, n_win, P = e.signatures(rows, sats, A, prompts=True)
    for r, s in enumerate(sats):
        c1, n1, P1 = e.signatures(rows, [s], A, prompts=True)
        _same(c1[0], cov[r]), _same(P1[0][:, :n1[0]], P[r][:, :n_win[r]])
        assert n1[0] == n_win[r]
    order = [3, 1, 1, 0, 2]
    c2, n2, P2 = e.signatures(rows, [sats[i] for i in order], A, prompts=True)
    for k, i in enumerate(order):
        _same(c2[k], cov[i]), _same(P2[k], P[i])
    # A = 3's antennas 0 .. 1 are A = 2's on the same rows (at 16368: 4 and 2), and so on down from the largest
    for small in R.KERNEL_ANTENNAS[cs]:
        cs_, ns_, Ps_ = e.signatures(rows_of(cs, small, False), sats, small, prompts=True)
        _same(Ps_, P[:, :small]), _same(cs_, cov[:, :small, :small]), _same(ns_, n_win)


def test_identical_rows_give_identical_prompt_rows(engines):
    for raw in (False, True):
        e = engines(2048, raw)
        x = rows_of(2048, 1, raw)[0]
        cov, n_win, P = e.signatures(np.stack([x] * 8), R.kernel_records(2048), 8, prompts=True)
        for a in range(1, 8):
            _same(P[:, a], P[:, 0])
        for r in range(len(cov)):
            assert np.all(cov[r] == cov[r, 0, 0]) and np.all(cov[r].imag == 0)


@pytest.mark.parametrize('cs', [2048, 16368])
def test_n_ms_cuts_the_windows(engines, cs):
    e = engines(cs, False)
    sats = R.kernel_records(cs)
    rows = rows_of(cs, 2, False)
    cov, n_win, P = e.signatures(rows, sats, 2, prompts=True)
    c3, n3, P3 = e.signatures(rows, sats, 2, n_ms=3, prompts=True)
    assert n3.tolist() == [3] * 4 and P3.shape == (4, 2, 3)
    _same(P3, P[:, :, :3])
    _, C_ref, _ = R.kernel_reference(cs, 2, 3)
    assert max(np.abs(c3[r] - C_ref[r]).max() / np.trace(C_ref[r]).real for r in range(4)) <= TOL[cs]['cov']
    c9, n9 = e.signatures(rows, sats, 2, n_ms=9)                 # more than fit: all of them
    _same(c9, cov), _same(n9, n_win)


def test_refusals_leave_the_handle_usable():
    """What needs the handle to be refused -- a PRN without a replica -- and that a search returns
    the same table before and after any of it."""
    from gpsmi import _lib
    from gpsmi.engine import AcqEngine, Config, EngineError
    e = AcqEngine(Config(**CFG[2048]))
    rows = rows_of(2048, 3, False)
    n = rows.shape[1]
    prns, freqs = [4, 5, 9, 11], [400.0, 3000.0, -4400.0]
    try:
        before = e.search_deep(rows[0][:5 * 2048], prns, freqs, 1, 5)
        cov, n_win = e.signatures(rows, R.kernel_records(2048), 3)
        _same(e.search_deep(rows[0][:5 * 2048], prns, freqs, 1, 5), before)
        sat = np.zeros(1, _lib.SIG_SAT_DTYPE)
        sat[0] = (17, 0, 100.0, 3.0)
        c, w = np.zeros((1, 3, 3), np.complex128), np.zeros(1, np.int32)
        cfg = _lib.SigCfg(3, 0, 0.0, 0.0)
        import ctypes as C
        rc = e.lib.gpsmi_acq_signature(e.h, _lib.ptr(rows), n, _lib.ptr(sat), 1, C.byref(cfg), _lib.ptr(c), _lib.ptr(w), None)
        assert rc == -3 and 'PRN 17' in e.lib.gpsmi_last_error().decode()
        rc = e.lib.gpsmi_acq_signature(e.h, _lib.ptr(rows), n, _lib.ptr(sat), 1, C.byref(cfg), None, _lib.ptr(w), None)
        assert rc == -1 and 'null' in e.lib.gpsmi_last_error().decode()
        for bad in ([(4, np.nan, 0.0)], [(4, 0.0, np.inf)], [(40, 0.0, 0.0)], []):
            with pytest.raises(EngineError):
                e.signatures(rows, bad, 3)
        with pytest.raises(ValueError):
            e.signatures(rows, R.kernel_records(2048), 2)         # three rows are not two antennas
        c2, n2 = e.signatures(rows, R.kernel_records(2048), 3)
        _same(c2, cov), _same(n2, n_win)
        _same(e.search_deep(rows[0][:5 * 2048], prns, freqs, 1, 5), before)
    finally:
        e.close()
