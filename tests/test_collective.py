"""Collective detection (gpsmi_acq_collective), the parts that need no GPU: the ABI's
declarations, struct sizes and plan; the numpy restatement (collective_ref.py) on planted peaks; the
host geometry; and the weak scene on the restated search.

The scene (collective_ref.weak_scene: snapshot_truth's strong geometry, eight satellites over 1 s,
all at one C/N0; a-priori 10 km and 1 s off) was stepped down from 30 dB-Hz in 1 dB steps:

    C/N0 dB-Hz   satellites over measure()'s threshold   collective search   fix error
        30                    8                           true cell            19.9 m
        27                    8                           true cell            18.0 m
        26                    7                           true cell            17.1 m
        25                    5                           true cell            15.7 m
        24                    3                           true cell            14.7 m

24 dB-Hz is the first level at which fewer than five satellites pass while the collective search
still lands on the true cell: SCENE_CN0.  "True cell": at the coarsest level the best cell is the
grid point nearest to the truth in east, north and time; at the last level (73 m, 0.045 s) it is the
nearest in east and north.  The last level's time step is a quarter of a sample of the fastest
satellite's lag, less than a phase error at this C/N0, so the time is only asked to be within one
step of the coarsest level (0.36 s) there; coarse_time_fix solves for it afterwards."""
import ctypes as C

import numpy as np
import pytest

import collective_ref as R

SCENE_CN0 = 24.0
SCENE_PASSING = {25.0: 5, 24.0: 3}                   # satellites over the threshold, restated
SCENE_FIX_ERROR_M = 14.67                            # the restatement's fix error at SCENE_CN0


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- ABI --------------------------------------------------------------------------------------------

def test_struct_sizes():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(17) == _lib.COLLECTIVE_SAT_DTYPE.itemsize == R.SAT_DTYPE.itemsize == 48
    assert lib.gpsmi_abi_sizeof(18) == C.sizeof(_lib.CollectiveGrid) == 64
    assert lib.gpsmi_abi_sizeof(19) == _lib.COLLECTIVE_CELL_DTYPE.itemsize == R.CELL_DTYPE.itemsize == 8
    assert lib.gpsmi_abi_sizeof(20) == -1
    for dt in (_lib.COLLECTIVE_SAT_DTYPE, _lib.COLLECTIVE_CELL_DTYPE):
        assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize       # no implicit padding
    assert _lib.COLLECTIVE_SAT_DTYPE == R.SAT_DTYPE and _lib.COLLECTIVE_CELL_DTYPE == R.CELL_DTYPE
    covered = sum(getattr(_lib.CollectiveGrid, n).size for n, _ in _lib.CollectiveGrid._fields_)
    assert covered == C.sizeof(_lib.CollectiveGrid)
    for name in ('gpsmi_acq_search_deep_rows_dev', 'gpsmi_acq_collective_dev', 'gpsmi_acq_collective_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _sats(n=3, **over):
    s = np.zeros(n, R.SAT_DTYPE)
    s['row'], s['bin_hi'] = np.arange(n), 2
    s['lag0'], s['g_e'], s['g_n'], s['g_t'] = 100.5, 0.005, -0.004, 3.0
    for k, v in over.items():
        s[k] = v
    return s


GRID = dict(n_e=67, n_n=33, n_t=2, pool=3, e0=-1000.0, n0=-500.0, t0=-1.0, d_e=30.0, d_n=30.0, d_t=2.0)


def _plan(cs, nsv_rows, nbins, sats, grid):
    from gpsmi import _lib
    from gpsmi.engine import collective_grid
    lib = _lib.load()
    g = collective_grid(**grid)
    scratch, wgs = C.c_size_t(7), C.c_int(-7)
    rc = lib.gpsmi_acq_collective_plan(cs, nsv_rows, nbins, _p(sats) if sats is not None else None,
                                       0 if sats is None else len(sats), C.byref(g), C.byref(scratch), C.byref(wgs))
    return rc, scratch.value, wgs.value, lib.gpsmi_last_error().decode()


def test_plan_sizes():
    """Scratch: the z rows, twice with a pooled copy; the launch: 64 grid points per workgroup."""
    cells = 67 * 33 * 2
    for cs in (2048, 16368):
        rc, scratch, wgs, msg = _plan(cs, 3, 3, _sats(), GRID)
        assert rc == 0, msg
        assert scratch == 2 * 3 * cs * 4 and wgs == (cells + 63) // 64
        rc, scratch, wgs, msg = _plan(cs, 3, 3, _sats(), dict(GRID, pool=1, n_e=1, n_n=1, n_t=1))
        assert (rc, scratch, wgs) == (0, 3 * cs * 4, 1), msg
    from gpsmi.engine import collective_plan
    assert collective_plan(2048, 3, 3, _sats(), GRID) == (2 * 3 * 2048 * 4, (cells + 63) // 64)


def test_plan_refusals():
    E_ARG, E_UNSUPPORTED = -1, -5
    ok = _sats()
    assert _plan(2048, 3, 3, ok, GRID)[0] == 0
    assert _plan(4096, 3, 3, ok, GRID)[0] == E_UNSUPPORTED                 # code_samples 2048 / 16368 only
    assert _plan(2048, 3, 3, None, GRID)[0] == E_ARG                         # null
    assert _plan(2048, 3, 3, ok[:0], GRID)[0] == E_ARG                       # nsat 1..32
    assert _plan(2048, 37, 3, _sats(33), GRID)[0] == E_ARG
    assert _plan(2048, 37, 3, _sats(32), GRID)[0] == 0
    assert _plan(2048, 0, 3, ok, GRID)[0] == E_ARG and _plan(2048, 38, 3, ok, GRID)[0] == E_ARG
    assert _plan(2048, 3, 0, ok, GRID)[0] == E_ARG
    assert _plan(2048, 2, 3, ok, GRID)[0] == E_ARG                           # row 2 of two rows
    assert _plan(2048, 3, 3, _sats(row=-1), GRID)[0] == E_ARG
    assert _plan(2048, 3, 2, ok, GRID)[0] == E_ARG                           # bin_hi 2 of two bins
    assert _plan(2048, 3, 3, _sats(bin_lo=3, bin_hi=2), GRID)[0] == E_ARG    # lo > hi
    assert _plan(2048, 3, 3, _sats(bin_lo=-1), GRID)[0] == E_ARG
    assert _plan(2048, 3, 3, _sats(bin_lo=2, bin_hi=2), GRID)[0] == 0        # one bin
    for k in ('lag0', 'g_e', 'g_n', 'g_t'):
        for bad in (np.nan, np.inf):
            assert _plan(2048, 3, 3, _sats(**{k: bad}), GRID)[0] == E_ARG
    for k in ('e0', 'n0', 't0', 'd_e', 'd_n', 'd_t'):
        assert _plan(2048, 3, 3, ok, dict(GRID, **{k: np.nan}))[0] == E_ARG
        assert _plan(2048, 3, 3, ok, dict(GRID, **{k: -np.inf}))[0] == E_ARG
    for k in ('n_e', 'n_n', 'n_t'):
        assert _plan(2048, 3, 3, ok, dict(GRID, **{k: 0}))[0] == E_ARG
    assert _plan(2048, 3, 3, ok, dict(GRID, pool=0))[0] == E_ARG and _plan(2048, 3, 3, ok, dict(GRID, pool=65))[0] == E_ARG
    assert _plan(2048, 3, 3, ok, dict(GRID, pool=64))[0] == 0
    # predicted lags stay below 2^30 samples
    assert _plan(2048, 3, 3, _sats(lag0=2.0 ** 30), GRID)[0] == E_ARG
    assert _plan(2048, 3, 3, _sats(g_e=2.0 ** 21), GRID)[0] == E_ARG         # * 1010 m
    assert _plan(2048, 3, 3, _sats(g_e=2.0 ** 19), GRID)[0] == 0
    # the cell count is bounded, and said so: 2^22 grid points
    rc, _, _, msg = _plan(2048, 3, 3, ok, dict(GRID, n_e=2048, n_n=2048, n_t=2))
    assert rc == E_UNSUPPORTED and '4194304' in msg
    assert _plan(2048, 3, 3, ok, dict(GRID, n_e=2048, n_n=2048, n_t=1))[0] == 0
    assert _plan(2048, 3, 3, ok, dict(GRID, n_e=2 ** 31 - 1, n_n=2 ** 31 - 1, n_t=2 ** 31 - 1))[0] == E_UNSUPPORTED


# ---- the restatement on planted peaks ---------------------------------------------------------------

def planted(cs, sats, E, N, T, c, seed=5, height=9.0):
    """Rows of small noise with one peak per satellite where (E, N, T, c) predicts it (bin_lo)."""
    rng = np.random.default_rng(seed)
    rows = (1.0 + 0.01 * rng.standard_normal((len(sats), 3, cs))).astype(np.float32)
    for s in sats:
        x = s['lag0'] + s['g_e'] * E + s['g_n'] * N + s['g_t'] * T + c
        rows[s['row'], s['bin_lo'], int(np.floor(x + 0.5)) % cs] += np.float32(height)
    return rows


@pytest.mark.parametrize('cs', [2048, 16368])
def test_planted_peaks_are_recovered(cs):
    """Five satellites with peaks consistent with one (E, N, T, c): the map's only cell that collects
    all five is that one.  The gradients send x_p below zero for some satellites and past cs for
    others, and the clock lag wraps the rest."""
    rng = np.random.default_rng(11)
    sats = _sats(5)
    sats['bin_lo'], sats['bin_hi'] = [0, 1, 2, 0, 1], [0, 2, 2, 2, 1]
    sats['lag0'] = [-2.5 * cs - 0.25, 17.5, cs - 2.75, 5.0 * cs + 0.5, 900.0]
    sats['g_e'], sats['g_n'] = rng.uniform(-0.0068, 0.0068, (2, 5))
    sats['g_t'] = rng.uniform(-5.5, 5.5, 5)
    grid = dict(n_e=9, n_n=7, n_t=3, pool=1, e0=-2400.0, n0=-1800.0, t0=-1.0, d_e=600.0, d_n=600.0, d_t=1.0)
    ie, i_n, it, c = 7, 2, 2, cs - 3
    E, N, T = grid['e0'] + ie * grid['d_e'], grid['n0'] + i_n * grid['d_n'], grid['t0'] + it * grid['d_t']
    x = sats['lag0'] + sats['g_e'] * E + sats['g_n'] * N + sats['g_t'] * T + c
    assert x.min() < 0 and x.max() > 2 * cs                                  # negative, and wrapped more than once
    rows = planted(cs, sats, E, N, T, c)
    cells = R.collective(rows, sats, grid)
    assert cells.shape == (3, 7, 9)
    k = np.unravel_index(np.argmax(cells['score']), cells.shape)
    assert k == (it, i_n, ie) and cells['lag'][k] == c
    z = [R.normalise(rows, s) for s in sats]
    want = np.float32(0)
    for p in range(5):
        want = np.float32(want + z[p].max()) if p else z[p].max()
    assert cells['score'][k] == want                                          # float32, ascending p
    others = np.delete(cells['score'].ravel(), np.ravel_multi_index(k, cells.shape))
    assert others.max() < want - 0.5 * z[0].max()                             # no other cell collects all five


def test_ties_and_pooling():
    """Equal maxima: the smallest clock lag.  A pooled row holds the maximum of w lags from its own
    on, circularly; the clock lags then go in steps of w."""
    cs = 2048
    sats = _sats(1, lag0=0.0, g_e=0.0, g_n=0.0, g_t=0.0)
    sats['bin_hi'] = 0
    rows = np.ones((1, 1, cs), np.float32)
    rows[0, 0, [700, 1300, 2047]] = 5.0
    one = dict(n_e=1, n_n=1, n_t=1, pool=1, e0=0.0, n0=0.0, t0=0.0, d_e=0.0, d_n=0.0, d_t=0.0)
    assert R.collective(rows, sats, one)['lag'][0, 0, 0] == 700
    # pool 3 does not divide 2048: lags 0, 3, ..., 2046; the row of lag 2046 covers 2046, 2047 and 0
    zw = R.normalise(rows, sats[0], 3)
    z = R.normalise(rows, sats[0])
    assert zw[2046] == z[2047] and zw[2045] == z[2047] and zw[2044] < z[2047] and zw[698] == z[700]
    assert R.collective(rows, sats, dict(one, pool=3))['lag'][0, 0, 0] == 699    # 699 covers 699 .. 701
    # x exactly half way rounds up: floor(x + 0.5)
    sats['lag0'] = 0.5
    assert R.collective(rows, sats, one)['lag'][0, 0, 0] == 699


def test_flat_bins_are_skipped():
    """A bin whose std is zero is skipped; a satellite with nothing else adds zero."""
    cs = 2048
    rng = np.random.default_rng(3)
    rows = rng.random((2, 2, cs), dtype=np.float32)
    rows[0, 0] = 0.25                                                         # flat
    rows[1] = 7.0                                                             # both flat
    sats = _sats(2, lag0=0.0, g_e=0.0, g_n=0.0, g_t=0.0)
    sats['bin_hi'] = 1
    z0, z1 = R.normalise(rows, sats[0]), R.normalise(rows, sats[1])
    mean, sd = R.row_stats(rows[0, 1])
    assert np.array_equal(z0, (rows[0, 1] - mean) / sd) and not z1.any()
    cells = R.collective(rows, sats, dict(n_e=1, n_n=1, n_t=1, pool=1, e0=0., n0=0., t0=0., d_e=0., d_n=0., d_t=0.))
    assert np.isfinite(cells['score']).all() and cells['lag'][0, 0, 0] == int(np.argmax(z0))


def test_tree_sum_is_the_statistics_order():
    """At 2048 lags the sum is gpsmi_stats.h's: eight magnitudes per thread in ascending q, a pairwise
    tree over the 256 threads."""
    x = np.random.default_rng(1).random(2048, dtype=np.float32)
    s = x.reshape(8, 256)
    t = ((((((s[0] + s[1]) + s[2]) + s[3]) + s[4]) + s[5]) + s[6]) + s[7]
    while len(t) > 1:
        t = t[0::2] + t[1::2]
    assert R.tree_sum(x) == t[0]
    assert abs(float(R.tree_sum(x)) - x.astype(np.float64).sum()) <= 2048 * 2.0 ** -24 * 12


# ---- the host geometry ------------------------------------------------------------------------------

def test_model_is_the_range_models_gradient():
    """lag0 and the gradients of collective_model against differences of modelled_range, and the
    predicted Dopplers against the scene's."""
    import snapshot_truth as T
    from gpsmi import snapshot as S
    sc, info = T.strong()
    prns = sorted(info['ephs'])
    pos, t = T.TRUTH, info['t0_gps']
    m = S.collective_model(info['ephs'], prns, t, pos, 2048)
    east, north, up = S.enu_axes(pos)
    assert abs(east @ north) < 1e-12 and abs(up @ pos / np.linalg.norm(pos) - 1) < 1e-4
    k = 2048000.0 / S.P.GPS_C

    def lag(dp, dt):
        return np.array([k * S.modelled_range(info['ephs'][p], t + dt, pos + dp)[0] for p in prns])
    for name, dp, dt, h in (('g_e', east, 0.0, 100.0), ('g_n', north, 0.0, 100.0), ('g_t', 0 * east, 1.0, 0.1)):
        num = (lag(dp * h, dt * h) - lag(-dp * h, -dt * h)) / (2 * h)
        assert np.abs(num - m[name]).max() <= 1e-6 * max(1.0, np.abs(num).max()), name
    assert np.abs(np.mod(m['lag0'] - lag(0 * east, 0.0) + 1024, 2048) - 1024).max() < 1e-6
    f_true = T.truth_meas(sc, 0)['f_hz']
    assert np.abs(m['f_hz'] - f_true).max() < 2.0 and (m['elevation'] > 5.0).all()
    # the code starts the model predicts, up to the common clock term, are the scene's
    d = np.mod(T.truth_meas(sc, 0)['code_phase'] - m['lag0'], 2048)
    d = np.mod(d - d[0] + 1024, 2048) - 1024
    assert np.abs(d).max() < 0.05
    # levels: pool halves to 1, the horizontal step is w / 2 samples of range
    lv = S.collective_levels(15.0e3, 2.0, 2048, float(np.abs(m['g_t']).max()))
    assert [l[0] for l in lv] == [8, 4, 2, 1] and abs(lv[-1][1] - 0.5 * S.P.GPS_C / 2048000.0) < 1e-9
    assert lv[0][3] * lv[0][1] >= 2 * 15.0e3 and all(l[3] == 5 for l in lv[1:])


# ---- the weak scene on the restated search -------------------------------------------------------------

@pytest.fixture(scope='module')
def scene():
    from gpsmi.engine import Config
    sc, info, data = R.weak_scene(SCENE_CN0)
    prns, freqs, bins, rows = R.scene_search(data, info, Config())
    pos, t = R.scene_apriori(info)
    res = R.pyramid(rows, info['ephs'], prns, bins, t, pos, R.SCENE_RADIUS_M, R.SCENE_TIME_S)
    return sc, info, prns, freqs, bins, rows, res


def nearest_cell(level, info):
    """The grid point of a level nearest to the truth: (i_t, i_n, i_e)."""
    from gpsmi import snapshot as S
    g, (centre, t_c) = level['grid'], level['centre']
    east, north, _ = S.enu_axes(centre)
    d = info['truth'] - centre
    return (int(np.rint((info['t0_gps'] - t_c - g['t0']) / g['d_t'])), int(np.rint((d @ north - g['n0']) / g['d_n'])),
            int(np.rint((d @ east - g['e0']) / g['d_e'])))


def test_scene_threshold_fails_and_collective_search_lands(scene):
    from gpsmi import snapshot as S
    sc, info, prns, freqs, bins, rows, res = scene
    assert prns == [2, 5, 8, 10, 13, 16, 19, 21]
    n_pass = len(R.passing(rows, bins))
    d = res['ecef'] - info['truth']
    east, north, up = S.enu_axes(info['truth'])
    print('%.0f dB-Hz: %d of %d satellites over the threshold; collective optimum %.1f m east, %.1f m north, '
          '%.1f m up, %.3f s from the truth, margin %.1f' % (SCENE_CN0, n_pass, len(prns), d @ east, d @ north, d @ up,
                                                             res['t_gps'] - info['t0_gps'], res['margin']))
    assert n_pass == SCENE_PASSING[SCENE_CN0] and n_pass < S.MIN_SAT
    first, last = res['levels'][0], res['levels'][-1]
    assert first['best'] == nearest_cell(first, info)
    assert last['best'][1:] == nearest_cell(last, info)[1:]
    assert abs(d @ east) <= 0.5 * last['grid']['d_e'] and abs(d @ north) <= 0.5 * last['grid']['d_n']
    assert abs(res['t_gps'] - info['t0_gps']) <= first['grid']['d_t']
    assert res['margin'] >= S.COLLECTIVE_MARGIN_MIN
    # the measurements at the optimum: all eight, and the fix from them
    meas, z = S.collective_records(lambda p: rows[bins[p][0], bins[p][1]:bins[p][2] + 1], prns,
                                   [freqs[b[1]:b[2] + 1] for b in bins], res['model'], res['lag'], 2048)
    assert meas['prn'].tolist() == prns and (z >= S.COLLECTIVE_WINDOW_MIN).all()
    import snapshot_truth as T
    assert np.abs(T.phase_error(sc, meas)).max() <= 0.5
    fix = S.coarse_time_fix(meas, info['ephs'], res['t_gps'], res['ecef'])
    err = np.linalg.norm(fix.ecef - info['truth'])
    print('fix %.2f m from the truth, g %.3f' % (err, fix.g))
    assert fix.ok and len(fix.prns) == 8 and abs(err - SCENE_FIX_ERROR_M) <= 0.05 * SCENE_FIX_ERROR_M


def test_scene_level_above_still_passes_five():
    """SCENE_CN0 is the first level: one dB above, five satellites are still over the threshold."""
    from gpsmi.engine import Config
    _, info, data = R.weak_scene(SCENE_CN0 + 1.0)
    _, _, bins, rows = R.scene_search(data, info, Config())
    assert len(R.passing(rows, bins)) == SCENE_PASSING[SCENE_CN0 + 1.0] >= 5


def test_snapshot_fix_refuses_bad_options():
    from gpsmi import snapshot as S
    with pytest.raises(ValueError):
        S.snapshot_fix(None, None, {}, 0.0, pos=np.zeros(3), collective='sometimes')
    with pytest.raises(ValueError):
        S.snapshot_fix(None, None, {}, 0.0, pos=None, collective=True)
    assert S.Fix().path == 'measure'
