"""CPU: the calls of windows_cases.py are what their names say -- by the numpy restatements alone
(sig_ref, profile_ref, cancel_ref) -- and the C++ plans make the same windows of them: the counts by the
`_plan` exports (as test_signature.py, test_profile.py and test_cancel.py call them), the starts and
cancellation's edges by the window rule's own program (tests/host/windows_check.cpp, built and run as
test_windows_host.py does: the exports report counts only)."""
import numpy as np
import pytest

import cancel_ref as CR
import windows_cases as W
from gpsmi import _lib, engine
from test_cancel import _plan as cancel_plan
from test_windows_host import exe, run  # noqa: F401  (exe: the fixture that builds the program)

CALLS = W.all_calls()


def ids(c):
    return c.id


@pytest.mark.parametrize('cs', [2048, 16368])
def test_slips(cs):
    """The steps between a record's starts: two values a sample apart, the ones the case table lists."""
    for name in W.SLIP_NAMES:
        call = W.slip(name, cs)
        assert call.n == 21 * cs + 123
        for (prn, f, tau), starts in zip(call.records, W.sig_starts(call)):
            Tc = cs / call.scale(f)
            want = W.SLIP_STEPS.get((name, cs), {}).get(prn, {int(np.floor(Tc)), int(np.floor(Tc)) + 1})
            assert W.steps(starts) == want, (name, prn)
            assert len(starts) in (19, 20, 21) and 0.99 < call.scale(f) < 1.01
    assert round(W.slip('fast', cs).scale(3096.0), 5) == 1.00774 and round(W.slip('slow', cs).scale(-3900.0), 5) == 0.99025
    assert round(W.slip('offset_fast', cs).scale(3096.0), 5) == 1.00762
    assert round(W.slip('offset_slow', cs).scale(3096.0), 5) == 0.99112
    # the record at 0.44 fs: its carrier's increment, and its windows slip like the others
    prn, f, _ = W.slip('offset_slow', cs).records[1]
    assert prn == 9 and f / (1000.0 * cs) == 0.44
    # profiles: in every slip call a run of 5 windows holds steps of both lengths
    for name in W.SLIP_NAMES:
        call = W.slip(name, cs)
        p = W.prof_settings(call)[0]
        assert p.coh == 5
        runs = [r for per_rec in W.prof_starts(call, p.Lh, p.coh) for r in per_rec]
        assert len(runs) >= 3 and any(len(W.steps(r)) == 2 for r in runs), name


def test_cancellation_windows():
    lens = lambda w: [hi - lo for lo, hi, _, _ in w]                    # noqa: E731
    # natural, PRN 4 at 2048: the first window is [0, 16), exactly min_window
    assert W.cancel_wins(W.slip('natural', 2048))[0][0][:2] == (0, CR.MIN_WINDOW)
    for cs, r0 in ((2048, 20), (16368, 161)):
        # fast: a first window of one sample, which is skipped
        w = W.cancel_wins(W.slip('fast', cs))[0]
        assert w[0][:2] == (0, 1) and lens(w)[0] < CR.MIN_WINDOW
        # slow: the longest windows there are, 1.01 cs; the first is cut at sample 0, r0 samples into its period
        w = W.cancel_wins(W.slip('slow', cs))[0]
        top = int(np.floor(cs / 0.99025))
        assert set(lens(w)[1:-1]) == {top, top + 1} and w[0][0] == 0 and w[0][3] == r0 and w[0][1] == cs
        # r0 + u reaches cs for the last r0 samples of the cut window: the replica wraps inside it
        assert sum(w[0][3] + u >= cs for u in range(lens(w)[0])) == r0 >= 2
    assert max(lens(W.cancel_wins(W.slip('slow', 2048))[0])) == 2069 > 8 * 256          # a ninth trip of 256 threads
    # everywhere else r0 is 0 or 1 behind the first window, and no window asks for replica point 2 cs:
    # with the scale inside (0.99, 1.01) a window is at most 1.0102 cs long
    for call in CALLS:
        for w in W.cancel_wins(call):
            assert all(r in (0, 1) for *_, r in w[1:])
            assert max(r + hi - lo - 1 for lo, hi, _, r in w) < 2 * call.cs
            assert w[0][0] == 0 and w[-1][1] == call.n and all(a[1] == b[0] for a, b in zip(w, w[1:]))


@pytest.mark.parametrize('cs', [2048, 16368])
def test_many_windows(cs):
    """The windows per record at the three lengths, what they ask of the kernels, and the runs."""
    for n, counts in zip(W.MANY_N[cs], W.MANY_WINDOWS[cs]):
        call = W.many_at(cs, n)
        assert [len(s) for s in W.sig_starts(call)] == counts
        for n_ms in (8, 9, 17, 256, 257):
            assert [len(s) for s in W.sig_starts(call, n_ms)] == [min(c, n_ms) for c in counts]
    groups = lambda c: -(-max(c) // W.KSIG_GROUP)                         # noqa: E731
    if cs == 2048:
        c300, c257, c9 = W.MANY_WINDOWS[cs]
        assert [c % 8 for c in c300] == [4, 3, 3] and groups(c300) == 38               # partial last groups behind 37
        assert min(c300) > W.KSIG_STRIDE and c257[0] == W.KSIG_STRIDE + 1               # a second window per thread: one
        assert c257[1] == W.KSIG_STRIDE <= 8 * (groups(c257) - 1)                       # its 33rd workgroup has nothing to do
        assert c9 == [9, 8, 8] and groups(c9) == 2                                      # a full group and one window
        assert [len(s) for s in W.sig_starts(W.many_at(cs, W.STALE_N))] == [19, 18, 18]
        call = W.many(cs)
        assert [len(r) for r in W.prof_starts(call, 8, 1)] == [len(r) for r in W.prof_starts(call, 32, 1)] == [299] * 3
        assert [len(r) for r in W.prof_starts(call, 8, 20)] == [len(r) for r in W.prof_starts(call, 8, 20, 7)] == [14] * 3
        assert [len(r) for r in W.prof_starts(W.many_at(cs, W.STALE_N), 8, 1)] == [18] * 3
    else:
        c19, c17, c9 = W.MANY_WINDOWS[cs]
        assert groups(c19) == 3 and [c % 8 for c in c19] == [3, 3, 2]
        assert [c % 8 for c in c17] == [1, 1, 0] and min(c17) <= 8 * (groups(c17) - 1)
        assert [c % 8 for c in c9] == [1, 1, 0] and min(c9) <= 8 * (groups(c9) - 1)
        call = W.many(cs)
        assert [len(r) for r in W.prof_starts(call, 32, 3)] == [len(r) for r in W.prof_starts(call, 5, 3)] == [6] * 3


def test_late_windows():
    """A record's windows begin with the rows whatever period tau names, so n_ms = 3 (n_runs = 1) takes
    the first three: the late samples are in the whole call, whose last windows lie behind 1000 cs."""
    call = W.late()
    cs = call.cs
    assert call.n == 1004 * cs + 50 and all(tau >= 1000 * cs for _, _, tau in call.records)
    assert [len(s) for s in W.sig_starts(call)] == [1004, 1003]
    assert all(s[0] < cs and s[-1] >= 1002 * cs and sum(j >= 1000 * cs for j in s) >= 3 for s in W.sig_starts(call))
    assert all(len(s) == 3 and s[-1] < 3 * cs for s in W.sig_starts(call, 3))
    assert [r.shape for r in W.prof_starts(call, 8, 3)] == [(334, 3)] * 2
    assert all(r[-1, -1] >= 1000 * cs for r in W.prof_starts(call, 8, 3))
    assert [len(w) for w in W.cancel_wins(call)] == [1006, 1005]


@pytest.mark.parametrize('call', CALLS, ids=ids)
def test_plans_count_what_the_restatements_list(call):
    for n_ms in (0, 3, 257):
        n_win, max_w = engine.signature_plan(call.cs, call.n, list(call.records), 2, n_ms=n_ms, **call.opts)
        want = [len(s) for s in W.sig_starts(call, n_ms)]
        assert n_win.tolist() == want and max_w == max(want)
    for p in W.prof_settings(call):
        n_runs, max_r, K = engine.profiles_plan(call.cs, call.n, call.prof_records(p.skip), **p.kw, **call.opts)
        want = [len(r) for r in W.prof_starts(call, p.Lh, p.coh, p.skip, p.n_runs)]
        assert n_runs.tolist() == want and max_r == max(want) and K == 2 * p.Lh + 1
    rc, max_w, msg = cancel_plan(call.cs, call.n, list(call.records), _lib.CancelCfg(call.carrier_hz, call.f_offset, 0, 0))
    assert rc == 0, msg
    assert max_w == max(len(w) for w in W.cancel_wins(call))


@pytest.mark.parametrize('call', CALLS, ids=ids)
def test_the_window_rule_lists_the_same_windows(exe, call):  # noqa: F811
    """gpsmi_windows.h itself: the starts of signatures and profiles, and ceil and rint of
    cancellation's edges -- from them lo, hi and r0 = (lo - j) mod cs as cancel_plan forms them."""
    cs, n = call.cs, call.n
    head = lambda f, tau: [cs, n, f, tau, call.carrier_hz, call.f_offset]      # noqa: E731
    cases, want, per = [], [], []
    for _, f, tau in call.records:
        one = call._replace(records=((1, f, tau),))
        cases.append(['starts'] + head(f, tau) + [0, 0, 0])
        want.append(W.sig_starts(one)[0])
        per.append(1)
        for p in W.prof_settings(call):
            cases.append(['starts'] + head(f, tau) + [p.Lh, p.skip, p.n_runs * p.coh])
            want.append(W.prof_starts(one, p.Lh, p.coh, p.skip, p.n_runs)[0].ravel().tolist())
            per.append(p.coh)
    for g, w, c, m in zip(run(exe, cases), want, cases, per):
        assert g[:len(w)] == w and len(g) - len(w) < m, c           # (the program does not drop an incomplete run)
    edges = []
    wins = W.cancel_wins(call)
    for (_, f, tau), w in zip(call.records, wins):
        Tc = cs / call.scale(f)
        k0 = int(np.rint((w[0][2] - tau) / Tc))
        edges.append(['edges'] + head(f, tau) + [k0, len(w) + 1])
    for g, w in zip(run(exe, edges), wins):
        ceil, rint = g[0::2], g[1::2]
        made = [(min(max(lo, 0), n), min(hi, n), j) for lo, hi, j in zip(ceil, ceil[1:], rint)]
        assert [m + ((m[0] - m[2]) % cs,) for m in made] == w
