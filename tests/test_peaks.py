"""Auxiliary peaks (gpsmi_acq_peaks), the parts that need no GPU: the ABI's
declarations, struct sizes and plan; the numpy restatement (peaks_ref.py) on planted surfaces; and
the doubled scene on the restated search.

The doubled scene: 2048 samples per code period, 100 ms as 25 segments of 4 ms, 51 bins of 200 Hz.
Five satellites at 38 .. 60 dB-Hz, four of them doubled by a copy that is 3 dB stronger, 60.3 samples
later and 25 Hz higher, and one PRN that is absent.  Three conditions at k = 4, with the project's own
corr_min = 8: both copies of every doubled PRN are picks 0 and 1, within one lag of the truth; every
other pick stays at or below corr_min; the absent PRN has no pick over it."""
import ctypes as C

import numpy as np
import pytest

import collective_ref as CR
import peaks_ref as R

CORR_MIN = 8.0


# ---- ABI --------------------------------------------------------------------------------------------

def test_struct_sizes():
    from gpsmi import _lib, engine
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(24) == C.sizeof(_lib.PeaksCfg) == 16
    assert lib.gpsmi_abi_sizeof(25) == _lib.PEAKS_PICK_DTYPE.itemsize == R.PICK_DTYPE.itemsize == 16
    assert lib.gpsmi_abi_sizeof(26) == -1
    assert _lib.PEAKS_PICK_DTYPE == R.PICK_DTYPE == engine.PEAKS_PICK_DTYPE
    assert sum(R.PICK_DTYPE.fields[n][0].itemsize for n in R.PICK_DTYPE.names) == 16      # no implicit padding
    assert sum(getattr(_lib.PeaksCfg, n).size for n, _ in _lib.PeaksCfg._fields_) == 16
    for name in ('gpsmi_acq_peaks_dev', 'gpsmi_acq_peaks_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _plan(cs, nsv_rows, nbins, k=4, guard=-1, lo=0, hi=None, null=False):
    from gpsmi import _lib
    lib = _lib.load()
    c = _lib.PeaksCfg(k, guard, lo, nbins - 1 if hi is None else hi)
    scratch, wgs = C.c_size_t(7), C.c_int(-7)
    rc = lib.gpsmi_acq_peaks_plan(cs, nsv_rows, nbins, None if null else C.byref(c), C.byref(scratch), C.byref(wgs))
    return rc, scratch.value, wgs.value, lib.gpsmi_last_error().decode()


def test_plan_sizes():
    """Scratch: (mean, std) per cell, zmax and its bin per satellite and lag; the statistics launch: a
    workgroup per satellite and bin of the window."""
    for cs in (2048, 16368):
        rc, scratch, wgs, msg = _plan(cs, 31, 51)
        assert (rc, scratch, wgs) == (0, 31 * 51 * 8 + 31 * cs * 8, 31 * 51), msg
        rc, scratch, wgs, msg = _plan(cs, 3, 51, lo=10, hi=12)
        assert (rc, scratch, wgs) == (0, 3 * 51 * 8 + 3 * cs * 8, 9), msg
    from gpsmi.engine import peaks_plan
    assert peaks_plan(2048, 1, 51, k=8, guard_lags=0, bins=(5, 5)) == (51 * 8 + 2048 * 8, 1)


def test_plan_refusals():
    E_ARG, E_UNSUPPORTED = -1, -5
    assert _plan(2048, 3, 3)[0] == 0 and _plan(16368, 3, 3)[0] == 0
    for cs in (1024, 4096, 16384, 0):
        assert _plan(cs, 3, 3)[0] == E_UNSUPPORTED                         # code_samples 2048 / 16368 only
    assert _plan(2048, 3, 3, null=True)[0] == E_ARG
    assert _plan(2048, 0, 3)[0] == E_ARG and _plan(2048, 39, 3)[0] == E_ARG     # nsv_rows 1..38
    assert _plan(2048, 1, 3)[0] == 0 and _plan(2048, 38, 3)[0] == 0
    assert _plan(2048, 3, 0)[0] == E_ARG and _plan(2048, 3, 4097)[0] == E_ARG   # nbins 1..4096
    assert _plan(2048, 3, 1)[0] == 0 and _plan(2048, 3, 4096)[0] == 0
    assert _plan(2048, 3, 3, k=0)[0] == E_ARG and _plan(2048, 3, 3, k=9)[0] == E_ARG
    assert _plan(2048, 3, 3, k=1)[0] == 0 and _plan(2048, 3, 3, k=8)[0] == 0
    assert _plan(2048, 3, 3, guard=-2)[0] == E_ARG and _plan(2048, 3, 3, guard=1025)[0] == E_ARG
    assert _plan(2048, 3, 3, guard=1024)[0] == 0 and _plan(2048, 3, 3, guard=0)[0] == 0
    assert _plan(16368, 3, 3, guard=8184)[0] == 0 and _plan(16368, 3, 3, guard=8185)[0] == E_ARG
    assert _plan(2048, 3, 3, lo=-1)[0] == E_ARG and _plan(2048, 3, 3, lo=2, hi=1)[0] == E_ARG
    assert _plan(2048, 3, 3, hi=3)[0] == E_ARG and _plan(2048, 3, 3, lo=2, hi=2)[0] == 0
    rc, scratch, wgs, msg = _plan(2048, 3, 3, k=9)
    assert (scratch, wgs) == (7, -7) and 'gpsmi_acq_peaks' in msg           # a refusal writes nothing


def test_engine_plan_raises():
    from gpsmi.engine import EngineError, peaks_plan
    with pytest.raises(EngineError, match=r'\(-5\)'):
        peaks_plan(4096, 3, 3)
    with pytest.raises(EngineError, match=r'\(-1\)'):
        peaks_plan(2048, 3, 3, bins=(2, 1))


# ---- the restatement's own properties -------------------------------------------------------------------

def circ(a, b, cs):
    d = abs(int(a) - int(b))
    return min(d, cs - d)


@pytest.mark.parametrize('cs', [2048, 16368])
@pytest.mark.parametrize('guard', [0, -1, 100])
def test_picks_are_more_than_the_guard_apart_and_descend(cs, guard):
    S = np.random.default_rng(cs + guard).integers(0, 16, (3, cs)).astype(np.float32)
    picks, cols = R.peaks_one(S, 8, guard)
    g = R.default_guard(cs) if guard < 0 else guard
    assert np.all(picks['lag'] >= 0)
    for i in range(8):
        for j in range(i):
            assert circ(picks['lag'][i], picks['lag'][j], cs) > g
    assert np.all(np.diff(picks['z']) <= 0)
    z, used = R.surface_z(S, 0, 2)
    assert used.all()
    for pk, col in zip(picks, cols):
        assert pk['z'] == z[:, pk['lag']].max() == z[pk['bin'], pk['lag']] and pk['s'] == S[pk['bin'], pk['lag']]
        assert np.array_equal(col[0], S[:, pk['lag']]) and np.array_equal(col[1], z[:, pk['lag']])
    # pick 0 is the first index of the largest z, in the smallest bin that attains it
    first = int(np.flatnonzero(z.max(axis=0) == z.max())[0])
    assert picks['lag'][0] == first and picks['bin'][0] == int(np.flatnonzero(z[:, first] == z.max())[0])


def test_first_index_ties_and_skipped_bins():
    cs = 2048
    S = np.zeros((3, cs), np.float32)
    S[0] = S[2] = np.arange(cs) % 3
    S[0, [5, 900]] = S[2, [5, 900]] = 100.0
    S[1] = 7.0                                                     # std 0: skipped
    picks, cols = R.peaks_one(S, 4)
    assert list(picks['lag'][:2]) == [5, 900] and list(picks['bin'][:2]) == [0, 0]
    assert picks['z'][0] == picks['z'][1]
    assert np.all(cols[:, 1, 1] == 0) and np.all(cols[:, 0, 1] == 7.0)
    assert np.array_equal(cols[:, 1, 0], cols[:, 1, 2])
    picks, cols = R.peaks_one(S, 4, bins=(2, 2))                   # outside the window: S, and z = 0
    assert list(picks['bin'][:2]) == [2, 2] and np.all(cols[:, 1, 0] == 0) and cols[0, 0, 0] == 100.0


def test_no_pick():
    cs = 2048
    S = np.zeros((3, cs), np.float32)
    S[0] = np.arange(cs) % 5
    S[1] = 7.0
    none = np.zeros(4, R.PICK_DTYPE)
    none['lag'] = none['bin'] = -1
    for picks, cols in (R.peaks_one(S, 4, bins=(1, 2)), R.peaks_one(np.full((2, cs), 3.0, np.float32), 4)):
        assert np.array_equal(picks, none) and not cols.any()
    picks, cols = R.peaks_one(S, 4, guard=cs // 2)                 # the guard takes every lag
    assert picks['lag'][0] == 4 and np.array_equal(picks[1:], none[1:]) and not cols[1:].any()
    picks, _ = R.peaks_one(S, 8, guard=cs // 2 - 1)                # one lag stays free: the opposite one
    assert list(picks['lag'][:3]) == [4, 4 + cs // 2, -1]


def test_guard_wraps():
    cs, g = 2048, 4
    S = (np.arange(cs) % 3).astype(np.float32)[None, :].copy()
    S[0, 0], S[0, cs - 1], S[0, cs - g], S[0, cs - g - 1], S[0, 500] = 100.0, 90.0, 85.0, 60.0, 80.0
    assert list(R.peaks_one(S, 3)[0]['lag']) == [0, 500, cs - g - 1]


def test_column_rule_is_largest_peak_hits():
    """hits_of_picks takes the bin from the column: the largest S among the bins over the threshold."""
    from gpsmi.pipeline import hits_of_picks
    picks = np.zeros((1, 3), R.PICK_DTYPE)
    picks[0] = [(700, 2, 30.0, 5.0), (90, 1, 9.0, 2.0), (-1, -1, 0.0, 0.0)]
    cols = np.zeros((1, 3, 2, 4), np.float32)
    cols[0, 0] = [[4.0, 9.0, 5.0, 9.0], [7.0, 25.0, 30.0, 25.0]]   # bin 2 has the largest z, bin 1 the largest S
    cols[0, 1] = [[1.0, 2.0, 3.0, 1.0], [2.0, 9.0, 7.9, 1.0]]      # bin 2 has a larger S below the threshold
    hits = hits_of_picks(picks, cols, [17], [-200.0, 0.0, 200.0, 400.0], CORR_MIN)
    assert hits == [(30.0, 17, 0.0, 700), (9.0, 17, 0.0, 90)]
    assert R.column_bin(cols[0, 0], CORR_MIN) == 1 and R.column_bin(cols[0, 1], CORR_MIN) == 1
    assert hits_of_picks(picks, cols, [17], [-200.0, 0.0, 200.0, 400.0], 9.0) == [(30.0, 17, 0.0, 700)]


# ---- the doubled scene on the restated search ------------------------------------------------------

CS = 2048
# (PRN, Doppler Hz, delay samples, C/N0 dB-Hz); all but the strongest are doubled
AUTHENTIC = [(5, 1230.0, 300.4, 45.0), (8, -2710.0, 1500.7, 45.0), (13, 3390.0, 40.2, 42.0),
             (19, -450.0, 1999.6, 60.0), (21, 2100.0, 777.1, 38.0)]
DOUBLED = (5, 8, 13, 21)
ABSENT = 27
COPY_DB, COPY_LAGS, COPY_HZ = 3.0, 60.3, 25.0


def doubled_scene():
    from gpsmi import synth
    sats = [synth.Sat(prn=p, doppler=f, delay=d, amp=float(CR.scene_amp(c)), phase0=0.3 * p)
            for p, f, d, c in AUTHENTIC]
    sats += [synth.Sat(prn=p, doppler=f + COPY_HZ, delay=(d + COPY_LAGS) % CS, amp=float(CR.scene_amp(c + COPY_DB)),
                       phase0=1.1 * p) for p, f, d, c in AUTHENTIC if p in DOUBLED]
    return synth.Scene(sats=sats, seed=5, noise_sigma=0.35, code_samples=CS, n_cyc=32)


def test_doubled_scene():
    import gps_oracle as orc
    from gpsmi.synth import raw_to_c64
    n_coh, n_seg = 4, 25
    data = raw_to_c64(doubled_scene().block_raw(0, n=n_coh * n_seg * CS))
    freqs = [-5000.0 + 200.0 * i for i in range(51)]
    prns = [p for p, *_ in AUTHENTIC] + [ABSENT]
    rows = CR.deep_rows(data, freqs, prns, n_coh, n_seg, orc.Params())
    picks, _ = R.peaks(rows, 4)
    for j, p in enumerate(prns):
        print(p, [(int(k['lag']), freqs[k['bin']], round(float(k['z']), 1)) for k in picks[j]])
    for j, (p, f, d, c) in enumerate(AUTHENTIC):
        truth = [d] + ([(d + COPY_LAGS) % CS] if p in DOUBLED else [])
        head, rest = picks[j][:len(truth)], picks[j][len(truth):]
        for t in truth:                                            # each truth has a pick of its own
            assert sum(min(abs(k['lag'] - t), CS - abs(k['lag'] - t)) <= 1.0 for k in head) == 1, (p, t)
        assert np.all(head['z'] > CORR_MIN), p
        assert np.all(rest['z'] <= CORR_MIN), p
    assert np.all(picks[len(AUTHENTIC)]['z'] <= CORR_MIN)         # the absent PRN
