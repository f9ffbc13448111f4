"""Refinement of weak / deep hits (gpsmi_acq_refine), the parts that need no GPU: the float64
restatement (refine_ref.py) against the truth of the pinned deep scene, hit_at against synth's
delay model, and the ABI's declarations, struct sizes and argument errors.

The bounds on the restatement come from the float64 prototype the feature was specified with
(deep scene, 25.5 dB-Hz, n_ms 1000, +-120 Hz at 2 Hz): Doppler errors -2.9 .. +1.0 Hz, exact bit
edges, peak / median 3.74 .. 5.01 for the satellites and 1.29 .. 1.31 for the absent candidate,
C/N0 23.1 .. 24.5 dB-Hz.  Asserted: 6 Hz (twice the worst), ratio > 3.1 / < 1.9 (half the distance
to the 2.5 threshold on either side), C/N0 in [22, 26], code phase within 0.5 sample."""
import ctypes as C

import numpy as np
import pytest

from deep_ref import DEEP_HIGH, DEEP_ZERO, L1_HZ, deep_scene
import small_scene as S
from refine_ref import ABSENT, check_truth, refine_ref, scene_cases

N_MS = 1000
N_BLOCKS = 33


@pytest.fixture(scope='module')
def scene_data():
    return deep_scene().block(0, n=N_BLOCKS * 65536)


# ---- the restatement against the truth ----------------------------------------------------------

@pytest.mark.parametrize('case', ['A', 'B'])
def test_restatement_meets_the_truth(scene_data, case):
    first, hits, truth = scene_cases(deep_scene(), N_MS, 2048)[case]
    rec, grid, P = refine_ref(scene_data[first:], hits, N_MS, 2048)
    assert grid.shape == (6, 121, 20) and P.shape == (6, 3, N_MS)
    assert np.all(rec['n_bits'] == 49) and rec['prn'].tolist() == [h[0] for h in hits]
    assert [t[2] for t in truth] == [0 if case == 'A' else 13] * 5
    check_truth(rec, truth)
    for h in range(5):
        per_edge = np.sort(grid[h].max(axis=0))
        print('prn %d runner-up edge / best %.3f' % (hits[h][0], per_edge[-2] / per_edge[-1]))


def test_restatement_hit_near_sample_zero_takes_the_next_period(scene_data):
    """delay < tap: the first window would start before sample 0; the hit takes delay + cs, which
    moves every window by one code period and the edge by one millisecond."""
    sc = deep_scene()
    s = sc.sats[0]
    cut = int(s.delay)                                   # the code now starts at sample 0
    rec, _, _ = refine_ref(scene_data[cut:], [(s.prn, round(s.doppler / 200) * 200.0, 0)], N_MS, 2048)
    assert rec['edge_ms'][0] == 19 and abs(rec['f_hz'][0] - s.doppler) <= 6.0
    assert abs(rec['code_phase'][0]) <= 0.5


# ---- hit_at ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('seconds', [1, 10])
def test_hit_at_follows_synths_delay_model(seconds):
    """synth: delay(k) = delay + delay_rate * k, delay_rate = -doppler / 1575.42e6."""
    from gpsmi.acquisition import hit_at
    from gpsmi.engine import Config
    from gpsmi._lib import REFINE_OUT_DTYPE
    cfg = Config()
    sample = seconds * 2048000
    for prn, dop, delay in DEEP_HIGH + [DEEP_ZERO] + [(7, 4999.0, 2.2), (8, -4999.0, 2046.9)]:
        rec = np.zeros(1, REFINE_OUT_DTYPE)[0]
        rec['prn'], rec['f_hz'], rec['code_phase'] = prn, dop, delay
        true = (delay - dop / L1_HZ * sample) % 2048
        f, d = hit_at(rec, sample, cfg)
        assert f == dop and isinstance(d, int) and 0 <= d < 2048
        assert d == int(np.rint(true)) % 2048
        # a Doppler error of 3 Hz moves the code by 0.04 samples in 10 s: the delay stays within one
        rec['f_hz'] = dop + 3.0
        assert (hit_at(rec, sample, cfg)[1] - d + 1) % 2048 <= 2
    rec['code_phase'] = -1.0
    with pytest.raises(ValueError):
        hit_at(rec, sample, cfg)


# ---- ABI --------------------------------------------------------------------------------------------

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_struct_sizes():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(7) == C.sizeof(_lib.RefineHit) == _lib.REFINE_HIT_DTYPE.itemsize == 16
    assert lib.gpsmi_abi_sizeof(8) == C.sizeof(_lib.RefineCfg) == 48
    assert lib.gpsmi_abi_sizeof(9) == _lib.REFINE_OUT_DTYPE.itemsize == 64
    for dt in (_lib.REFINE_HIT_DTYPE, _lib.REFINE_OUT_DTYPE):            # no implicit padding
        assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize
    covered = sum(getattr(_lib.RefineCfg, n).size for n, _ in _lib.RefineCfg._fields_)
    assert covered == C.sizeof(_lib.RefineCfg)
    for name in ('gpsmi_acq_refine', 'gpsmi_acq_refine_dev', 'gpsmi_acq_refine_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_argument_errors_need_no_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    hits = np.zeros(65, _lib.REFINE_HIT_DTYPE)
    hits['prn'], hits['delay'], hits['freq_hz'] = 6, 412, -4800.0
    out = np.zeros(65, _lib.REFINE_OUT_DTYPE)
    buf = np.zeros(16, np.float32)
    n = 1002 * 2048 + 1

    def cfg(**kw):
        d = dict(n_ms=1000, tap_samples=0, df_step_hz=0.0, df_half_hz=0.0, carrier_hz=L1_HZ,
                 f_offset_hz=0.0, min_ratio=0.0, reserved=0)
        d.update(kw)
        return _lib.RefineCfg(**d)

    def plan(cs=2048, n=n, hits=hits, nhits=5, c=None, want=-1, text=None):
        n_df = C.c_int(-7)
        c = cfg() if c is None else c
        rc = lib.gpsmi_acq_refine_plan(cs, n, None if hits is None else _p(hits), nhits,
                                       C.byref(c) if c is not False else None, C.byref(n_df))
        assert rc == want, (rc, lib.gpsmi_last_error())
        if text:
            assert text in lib.gpsmi_last_error(), lib.gpsmi_last_error()
        return n_df.value

    assert plan(want=0) == 121                                  # the defaults: +-120 Hz at 2 Hz
    assert plan(c=cfg(df_step_hz=0.5, df_half_hz=255.75), want=0) == 1024
    assert plan(cs=16368, n=302 * 16368 + 8, c=cfg(n_ms=300), want=0) == 121
    assert plan(nhits=64, hits=hits, want=0) == 121
    # null pointers
    plan(hits=None, text=b'null')
    plan(c=False, text=b'null')
    for fn in (lib.gpsmi_acq_refine, lib.gpsmi_acq_refine_dev):
        assert fn(None, _p(buf), n, _p(hits), 5, C.byref(cfg()), _p(out), None, None) == -1
        assert b'null' in lib.gpsmi_last_error()
    # n_ms
    for bad in (0, 20, 30, 1010, -40):
        plan(c=cfg(n_ms=bad), text=b'multiple of 20')
    # too short n
    plan(n=n - 1, text=b'shorter')
    plan(cs=16368, n=302 * 16368 + 7, c=cfg(n_ms=300), text=b'shorter')
    # more than 1024 grid points
    plan(c=cfg(df_step_hz=0.5, df_half_hz=256.0), text=b'1024')
    # nhits
    plan(nhits=0, text=b'nhits')
    plan(nhits=65, text=b'nhits')
    # carrier_hz, f_offset_hz
    for bad in (float('nan'), 0.0, -1.0, float('inf')):
        plan(c=cfg(carrier_hz=bad), text=b'carrier_hz')
    plan(c=cfg(f_offset_hz=float('nan')), text=b'f_offset_hz')
    # hits
    for field, bad in (('prn', 0), ('prn', 38), ('delay', -1), ('delay', 2048), ('freq_hz', float('nan'))):
        h = hits.copy()
        h[field][3] = bad
        plan(hits=h, text=field.encode().split(b'_')[0])
    # a slide that leaves the data (f_offset of 60 MHz: 78 samples per millisecond)
    plan(c=cfg(f_offset_hz=60e6), text=b'leaves')
    # what is unsupported rather than wrong
    plan(cs=4096, want=-5)
    plan(n=8003 * 2048, c=cfg(n_ms=8020), want=-5, text=b'8000')
    assert plan(n=8003 * 2048, c=cfg(n_ms=8000), want=0) == 121


def test_header_states_the_cap():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, 'include', 'gpsmi.h')).read()
    m = re.search(r'#define\s+GPSMI_REFINE_MAX_MS\s+(\d+)', src)
    assert m and int(m.group(1)) >= 4000
    assert ABSENT[0] not in [p for p, _, _ in DEEP_HIGH + [DEEP_ZERO]]


# ---- the option and shape cases of small_scene.py: the restatement's decisions are not marginal ----

def _case_runs(case):
    return [False, True] if case.raw else [False]


@pytest.mark.parametrize('case', [c for c in S.REFINE_CASES if not c.zeros], ids=repr)
def test_small_scene_decisions_are_not_marginal(case):
    """The GPU test compares prn, n_bits, edge_ms, confirmed and code_phase == -1 exactly.  That is
    sound where the restatement's own decision is clear of its threshold: ratio outside 2.5 +- 0.25,
    the top two grid cells more than 1e-3 of the peak apart (2e-4 where the grid step cannot give
    more, see small_scene.py), tap_metric[0] and [2] more than 1e-3 of [1] away from it -- on the
    complex64 rendering and, where the case also runs from raw u8, on the decoded samples."""
    for decoded in _case_runs(case):
        ref, grid, P = case.ref(decoded)
        ok, text = S.refine_margins(ref, grid, case.gap)
        print('%s%s\n%s' % (case.name, ' (decoded u8)' if decoded else '', text))
        assert ok
        assert np.all(ref['n_bits'] == case.n_ms // 20 - 1) and P.shape == (len(case.hits), 3, case.n_ms)


def test_small_scene_cases_reach_what_they_are_for():
    """The shapes and branches each case exists for, read off the restatement."""
    by = {c.name: c for c in S.REFINE_CASES}
    B = lambda name: by[name].n_ms // 20 - 1
    assert [B('min-2048'), B('lanes-1300'), B('lanes-1320'), B('threads-5140'), B('threads-5160')] == [1, 64, 65, 256, 257]
    assert by['tail-60'].n_ms % 8 == by['tail-100'].n_ms % 8 == 4 and by['max-8000'].n_ms == 8000
    n_df = [by[n].ref()[1].shape[1] for n in ('n_df-1-0.4', 'n_df-1-1', 'n_df-2-2', 'n_df-0.5-255.75')]
    assert n_df == [1, 3, 3, 1024]
    ref, grid, _ = by['n_df-0.5-255.75'].ref()
    for h in range(len(ref)):                             # an interior peak: the parabola runs
        d = int(np.argmax(grid[h])) // 20
        assert 0 < d < 1023
    for name, row in (('rows-first', 0), ('rows-last', 8)):
        ref, grid, _ = by[name].ref()
        assert grid.shape[1] == 9
        for h in range(len(ref)):
            assert int(np.argmax(grid[h])) // 20 == row
            assert ref['f_hz'][h] == by[name].hits[h][1] + (-20.0 + 5.0 * row)      # no parabola
    assert [h[2] for h in by['tap-512'].hits] == [0, 511, 512, 2047] and by['tap-512'].n == 62 * 2048 + 512
    assert len(by['many-64'].hits) == 64 and len({h[1:] for h in by['many-64'].hits}) == 64
    ref, _, _ = by['misaligned'].ref()
    assert np.all(ref['code_phase'] == -1.0)
    ok = by['tail-100'].ref()[0]
    assert np.all(ok['code_phase'] >= 0) and np.all(ok['edge_ms'] == by['tail-100'].edge)
    for name in ('slide-minus-2048', 'slide-plus-2048', 'slide-minus-16368', 'slide-plus-16368'):
        c = by[name]                                      # windows sliding several samples per ms
        slide = -(c.hits[0][1] - c.opts['f_offset']) / L1_HZ * c.cs
        assert abs(slide) > 3.0 and (slide > 0) == (c.opts['f_offset'] > 0)


def test_small_scene_zeros_is_the_degenerate_record():
    case = next(c for c in S.REFINE_CASES if c.zeros)
    ref, grid, P = case.ref()
    assert not grid.any() and not P.any()
    for r, (prn, freq, delay) in zip(ref, case.hits):
        assert (r['prn'], r['edge_ms'], r['n_bits'], r['confirmed']) == (prn, 0, 1, 0)
        assert r['f_hz'] == freq - 120.0 and r['peak'] == r['median'] == 0.0 and np.isnan(r['ratio'])
        assert r['code_phase'] == delay and r['mu'] == 0.0 and np.isnan(r['cn0_dbhz'])
