"""gpsmi.snapshot on the CPU: the coarse-time solver, the Doppler a-priori and the measurement
records on truth measurements of synth_nav.geometric_scene(README position, 1.0 s, n_sats=8,
seed=79) (snapshot_truth.py), and the whole chain on the float64 restatements of the three GPU
stages (deep_ref / refine_ref / wtrk_ref), which gives the reference fix errors of
test_gpu_snapshot.py.  No GPU.

Measured with the committed solver (printed by the tests): truth fix 0.0083 m from the scene's
truth, time 9.5 us off (the scene's own polynomial fit error is 6.3e-5 sample = 9 mm of range);
doppler_fix with +-3 Hz noise and a +700 Hz offset lands at most 7.3 km from the truth at time
errors 0 / +-30 s; five satellites on truth 0.016 m (g 2.84).  Restatement chain, fix error and geometry factor g:

    scene                      source   error      g
    strong, 1.0 s              refine    17.62 m   1.91
    strong, 1.0 s              track      7.69 m   1.91
    mixed, 1.2 s               refine  1116.2 m   22.95
    mixed, 1.2 s               track    419.6 m   22.94
    strong, 131072 samples     refine    10.98 m   1.91
"""
import functools
import os
import sys

import numpy as np
import pytest

import snapshot_truth as T
from gpsmi import snapshot as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 2048000.0
M_PER_SAMPLE = S.P.GPS_C / FS
TRUTH_ERR_M = 0.0083                     # measured, see the module docstring
CAP_M = 1.0
MID = 1024000


def apriori(rng, dist):
    u = rng.normal(size=3)
    return T.TRUTH + dist * u / np.linalg.norm(u)


@functools.lru_cache(maxsize=None)
def truth_fix():
    sc, info = T.strong()
    m = T.truth_meas(sc, MID)
    m.setflags(write=False)
    return m, S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, MID), T.TRUTH)


def test_truth_fix():
    _, info = T.strong()
    m, fx = truth_fix()
    err = np.linalg.norm(fx.ecef - T.TRUTH)
    print('truth fix: %.4f m, time %+.2e s, g %.3f, integers %s' % (err, fx.t_gps - T.t_gps_of(info, MID), fx.g, fx.integers))
    assert fx.ok and sorted(fx.prns) == [2, 5, 8, 10, 13, 16, 19, 21]
    assert err <= min(2 * TRUTH_ERR_M, CAP_M)
    assert abs(fx.t_gps - T.t_gps_of(info, MID)) <= 1.0e-3
    assert fx.sample == MID and abs(fx.bias_m) <= S.C_MS / 2 and len(fx.residuals) == len(fx.integers) == 8
    # explicit weights: the heaviest satellite is the reference; the scene's 4-mm residuals weighted
    # otherwise move the fix by millimetres
    w = np.ones(8)
    w[5] = 2.0
    fw = S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, MID), T.TRUTH, weights=w)
    assert fw.ok and fw.ref_prn == 16 and fw.integers[5] == 0 and np.linalg.norm(fw.ecef - fx.ecef) <= 0.01


@pytest.mark.parametrize('dist,dt', [(50.0e3, 30.0), (50.0e3, -30.0), (75.0e3, 0.0), (0.0, 90.0)])
def test_convergence_region(dist, dt):
    _, info = T.strong()
    m, ref = truth_fix()
    rng = np.random.default_rng(int(dist + 7 * dt) + 1000)
    for _ in range(12):
        fx = S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, MID) + dt, apriori(rng, dist))
        assert fx.ok, fx.reason
        assert np.linalg.norm(fx.ecef - ref.ecef) <= 1.0e-3
        assert np.array_equal(fx.integers, ref.integers)


@pytest.mark.parametrize('dist,dt', [(300.0e3, 0.0), (0.0, 180.0), (0.0, -180.0)])
def test_beyond_the_region_is_refused_or_right(dist, dt):
    _, info = T.strong()
    m, ref = truth_fix()
    rng = np.random.default_rng(5)
    n_ok = 0
    for _ in range(12):
        fx = S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, MID) + dt, apriori(rng, dist))
        if fx.ok:
            n_ok += 1
            assert np.linalg.norm(fx.ecef - T.TRUTH) <= CAP_M
        else:
            assert fx.ecef is None and fx.reason
    print('%g km %+g s: %d of 12 right, the others refused' % (dist / 1e3, dt, n_ok))


@pytest.mark.parametrize('which', [0, 3])            # the reference satellite (the first of equals), another
@pytest.mark.parametrize('edge', ['zero', 'cs'])
@pytest.mark.parametrize('grid', ['as it falls', 'at the satellite'])
def test_integer_step_at_the_wrap(which, edge, grid):
    """A code start within 0.01 sample behind (`zero`) or ahead of (`cs`) the measurement sample,
    +-0.02 sample of noise on it, the code phase reported modulo cs as a receiver would, so that
    it jumps by cs between the two signs; the fix must not move beyond the noise times g (one
    satellite moved by d moves the unit-weight fix by at most g d).  The solver's own
    millisecond grid lies where the a-priori time puts it: `at the satellite` moves that time
    (10 s off, by less than 1 ms more) until the grid's wrap falls on this satellite's code start
    as well, and the integers of the two signs then differ by one.  Measured: 0.88 .. 1.88 m
    against 5.58 m."""
    from weaknav_truth import arrival
    sc, info = T.strong()
    cs = sc.code_samples
    sat = sorted(sc.sats, key=lambda s: s.prn)[which]
    k = arrival(sat, np.arange(300, 700), cs)
    frac = k - np.floor(k)
    if edge == 'zero':
        i = int(np.argmax((frac > 0.001) & (frac < 0.009)))
        sample = int(np.floor(k[i]))
    else:
        i = int(np.argmax((frac > 0.996) & (frac < 0.999)))
        sample = int(np.ceil(k[i]))
    m = T.truth_meas(sc, sample)
    j = int(np.flatnonzero(m['prn'] == sat.prn)[0])
    near = m['code_phase'][j] if edge == 'zero' else cs - m['code_phase'][j]
    print('prn %d sample %d code phase %.4f' % (sat.prn, sample, m['code_phase'][j]))
    assert 0.0 <= near < 0.01
    clean = S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, sample), T.TRUTH)
    assert clean.ok and np.linalg.norm(clean.ecef - T.TRUTH) <= CAP_M
    bound = clean.g * 0.02 * M_PER_SAMPLE
    t0 = T.t_gps_of(info, sample) + 10.0
    if grid == 'at the satellite':
        t0 -= (t0 % 1.0e-3 + m['code_phase'][j] / FS) % 1.0e-3
    ints, phases = [], []
    for noise in (-0.02, 0.02):
        mm = m.copy()
        mm['code_phase'][j] = (mm['code_phase'][j] + noise) % cs
        phases.append(mm['code_phase'][j])
        fx = S.coarse_time_fix(mm, info['ephs'], t0, apriori(np.random.default_rng(3), 30.0e3))
        assert fx.ok, fx.reason
        moved = np.linalg.norm(fx.ecef - clean.ecef)
        print('noise %+.2f -> code phase %.4f, moved %.3f m (bound %.3f m), integers %s' % (
            noise, mm['code_phase'][j], moved, bound, fx.integers))
        assert moved <= bound
        ints.append(fx.integers[j] if which else fx.integers[(j + 1) % 8])
    assert abs(abs(phases[0] - phases[1]) - cs) <= 0.04          # (the code phase did wrap)
    if grid == 'at the satellite':
        assert abs(ints[0] - ints[1]) == 1                       # (and there the integer with it)


def test_five_and_four_satellites():
    sc, info = T.strong()
    m, _ = truth_fix()
    five = S.coarse_time_fix(m[[0, 2, 4, 5, 7]], info['ephs'], T.t_gps_of(info, MID) + 20.0, apriori(np.random.default_rng(9), 30.0e3))
    print('five satellites: %.4f m, g %.2f' % (np.linalg.norm(five.ecef - T.TRUTH), five.g))
    assert five.ok and len(five.prns) == 5 and np.linalg.norm(five.ecef - T.TRUTH) <= CAP_M
    four = S.coarse_time_fix(m[:4], info['ephs'], T.t_gps_of(info, MID), T.TRUTH)
    assert not four.ok and four.ecef is None and '5 needed' in four.reason
    # five satellites leave nothing to test the integers with: far from the a-priori is refused
    far = S.coarse_time_fix(m[[0, 2, 4, 5, 7]], info['ephs'], T.t_gps_of(info, MID), apriori(np.random.default_rng(9), 100.0e3))
    assert not far.ok or np.linalg.norm(far.ecef - T.TRUTH) <= CAP_M


@pytest.mark.parametrize('which', [0, 3])
def test_dropped_satellite(which):
    _, info = T.strong()
    m, _ = truth_fix()
    mm = m.copy()
    mm['code_phase'][which] = (mm['code_phase'][which] + 300.0) % 2048
    fx = S.coarse_time_fix(mm, info['ephs'], T.t_gps_of(info, MID) + 10.0, apriori(np.random.default_rng(4), 20.0e3))
    assert fx.ok, fx.reason
    assert fx.dropped == [int(m['prn'][which])] and len(fx.prns) == 7
    assert np.linalg.norm(fx.ecef - T.TRUTH) <= CAP_M
    # ... and two such satellites are more than the test may take out
    mm['code_phase'][5] = (mm['code_phase'][5] + 500.0) % 2048
    fx = S.coarse_time_fix(mm, info['ephs'], T.t_gps_of(info, MID), T.TRUTH)
    assert not fx.ok and fx.ecef is None


SIX = [(1, 2, 3, 5, 6, 7), (0, 1, 2, 3, 4, 5), (0, 2, 3, 4, 5, 7), (0, 2, 3, 4, 6, 7), (2, 3, 4, 5, 6, 7)]


@pytest.mark.parametrize('sub', SIX)
def test_six_satellites_and_one_bad_measurement(sub):
    """Six satellites leave one degree of freedom: nothing is dropped (five would fit anything),
    a solution that fails the residual test is refused, and a bad measurement the one residual
    direction does not see moves the fix by no more than its own protect_m says.  Every satellite
    of the six in turn 20, 100 and 300 samples off, the a-priori 5 km and 5 s off.  (Over all 28
    subsets 25 of the 504 cases pass the test with a wrong fix, the largest 35.5 km, each within
    its protect_m, the closest at 0.98 of it.)"""
    _, info = T.strong()
    m, _ = truth_fix()
    pos = apriori(np.random.default_rng(2), 5.0e3)
    n_ok = n_refused = 0
    worst = 0.0
    for k in range(6):
        for off in (20.0, 100.0, 300.0):
            mm = m[list(sub)].copy()
            mm['code_phase'][k] = (mm['code_phase'][k] + off) % 2048
            fx = S.coarse_time_fix(mm, info['ephs'], T.t_gps_of(info, MID) + 5.0, pos)
            assert fx.dropped == []
            if not fx.ok:
                n_refused += 1
                assert fx.ecef is None and fx.reason
                continue
            n_ok += 1
            err = np.linalg.norm(fx.ecef - T.TRUTH)
            worst = max(worst, err / fx.protect_m)
            assert err <= CAP_M or err <= fx.protect_m
    print('%s: %d refused, %d passed the test, the worst of those at %.2f of its protect_m' % (sub, n_refused, n_ok, worst))
    assert n_refused >= 12
    clean = S.coarse_time_fix(m[list(sub)], info['ephs'], T.t_gps_of(info, MID) + 5.0, pos)
    assert clean.ok and np.linalg.norm(clean.ecef - T.TRUTH) <= CAP_M and np.isfinite(clean.protect_m)


def test_doppler_fix_lands_inside_the_region():
    sc, info = T.strong()
    _, ref = truth_fix()
    m = T.truth_meas(sc, MID)
    rng = np.random.default_rng(11)
    worst = 0.0
    for dt in (0.0, 30.0, -30.0):
        for _ in range(4):
            mm = m.copy()
            mm['f_hz'] += 700.0 + rng.uniform(-3.0, 3.0, len(mm))
            pos, drift = S.doppler_fix(mm, info['ephs'], T.t_gps_of(info, MID) + dt)
            worst = max(worst, np.linalg.norm(pos - T.TRUTH))
            assert abs(drift - 700.0) < 30.0
            fx = S.coarse_time_fix(mm, info['ephs'], T.t_gps_of(info, MID) + dt, pos)
            assert fx.ok, fx.reason
            assert np.linalg.norm(fx.ecef - ref.ecef) <= 1.0e-3
    print('doppler_fix: worst distance from the truth %.0f m' % worst)
    with pytest.raises(ValueError):
        S.doppler_fix(m[:3], info['ephs'], T.t_gps_of(info, MID))


def test_ghost_rule():
    from refine_ref import REFINE_DTYPE
    rec = np.zeros(4, REFINE_DTYPE)
    rec['prn'], rec['confirmed'] = [4, 9, 17, 20], 1
    rec['f_hz'] = [1230.0, -2768.0, 3232.0, 1236.0]               # 9 and 17 lie on 4's lines, 20 does not
    rec['cn0_dbhz'] = [48.0, 36.0, 39.0, 30.0]
    assert S.drop_ghosts(rec).tolist() == [False, True, False, False]
    rec['cn0_dbhz'][1] = np.nan
    assert S.drop_ghosts(rec).tolist() == [False, True, False, False]


# ---------------------------------------------------------------- the restatement chain
@functools.lru_cache(maxsize=None)
def restated(name, n=None):
    """deep_ref / refine_ref / wtrk_ref on a scene, restricted to the true PRNs and their bins
    +-1, with measure()'s rules (largest peak over the threshold, refine_centred's re-centring, refined_records,
    tracked_records).  -> {source: records}."""
    import gps_oracle as orc
    import wtrk_ref as W
    from deep_ref import deep_bins, deep_table
    from refine_ref import refine_ref
    sc, info = {'strong': T.strong, 'mixed': T.mixed}[name]()
    data = T.c64(name)[:n]
    cs, n = sc.code_samples, len(data)
    n_seg = n // cs // 4
    found = []
    for s in sorted(sc.sats, key=lambda s: s.prn):
        bins = deep_bins(float(T.truth_meas(sc, 0, mid=n // 2, prns=[s.prn])['f_hz'][0]))
        tab = deep_table(data[:n_seg * 4 * cs], bins, [s.prn], 4, n_seg, orc.Params())
        nmc = (tab['peak'][:, 0] - tab['mean'][:, 0]) / tab['std'][:, 0]
        b = int(np.argmax(np.where(nmc > 8.0, tab['peak'][:, 0], -np.inf)))
        assert nmc[b] > 8.0
        found.append((float(nmc[b]), s.prn, bins[b], int(tab['argmax'][b, 0])))
    n_ms = ((n - 1) // cs - 2) // 20 * 20
    rec = refine_ref(data, [h[1:] for h in found], n_ms, cs)[0]
    for _ in range(2):
        bad = [i for i, r in enumerate(rec) if r['confirmed'] == 1 and r['code_phase'] < 0]
        for i in bad:
            nmc, s, f, d = found[i]
            e, _, l = rec[i]['tap_metric']
            found[i] = (nmc, s, f, int(d + (-1 if e > l else 1)) % cs)
        if bad:
            rec[bad] = refine_ref(data, [found[i][1:] for i in bad], n_ms, cs)[0]
    rec, found, out = S.refined_records(rec, found, cs)
    res = {'refine': out}
    if n >= 500 * cs:
        bits, states, _ = W.track_ref(data, [W.open_ref(r, cs) for r in rec], n // (20 * cs), cs)
        res['track'] = out.copy()
        S.tracked_records(res['track'], bits, [s['bit_no'] for s in states], n, cs)
    return res


def restated_fix(name, source, n=None):
    _, info = {'strong': T.strong, 'mixed': T.mixed}[name]()
    m = restated(name, n)[source]
    ref = int(np.argmax(S.cn0_weights(m['cn0_dbhz'])))
    pos, _ = S.doppler_fix(m, info['ephs'], info['t0_gps'] + 20.0)
    return m, S.coarse_time_fix(m, info['ephs'], info['t0_gps'] + 20.0 + m['sample'][ref] / FS, pos)


@pytest.mark.parametrize('name,n,n_sats', [('strong', None, 8), ('mixed', None, 6), ('strong', T.TWO_BLOCKS, 8)])
def test_restatement_chain(name, n, n_sats):
    """The reference fix errors (no a-priori position, time 20 s off): they must be the figures
    snapshot_truth.REF carries for the GPU tests, and 'track' must be the better source on both
    1-s scenes, as DEFAULT_SOURCE says."""
    sc, _ = {'strong': T.strong, 'mixed': T.mixed}[name]()
    err = {}
    for source, m in restated(name, n).items():
        m, fx = restated_fix(name, source, n)
        assert fx.ok and len(fx.prns) == n_sats and not fx.dropped, fx.reason
        err[source] = np.linalg.norm(fx.ecef - T.TRUTH)
        pe = T.phase_error(sc, m)
        print('%s %s %s: fix error %.2f m, g %.3f, worst code phase error %.3f sample, worst Doppler error %.2f Hz' % (
            name, n or '', source, err[source], fx.g, np.abs(pe).max(),
            np.abs(T.doppler_error(sc, m, (n or len(T.raw(name))) // 2)).max()))
        assert {s.decode() for s in m['source']} == {source}
        if n is None:
            ee = T.edge_error(sc, m)
            print('   bit edges: worst %.3f sample from a true one' % np.abs(ee).max())
            assert np.abs(ee).max() <= 0.5           # (the code phase's own error, no whole period)
        else:                                        # 60 ms: two bits do not place an edge
            assert np.isnan(m['edge']).all()
        assert abs(err[source] - T.REF[name, n, source][0]) <= 0.05 * T.REF[name, n, source][0]
        assert abs(fx.g - T.REF[name, n, source][1]) <= 0.01 * T.REF[name, n, source][1]
    if n is None:
        assert err['track'] < err['refine'] and S.DEFAULT_SOURCE == 'track'


def test_measure_refuses_what_it_cannot_do():
    from gpsmi.engine import Config

    class Acq:                                        # (nothing reaches the engine)
        cfg = Config()
    with pytest.raises(TypeError):
        S.measure(Acq(), (None, 2048000), colour='red')
    assert S.min_samples(2048) == 86017              # (refineHits' n_ms = 40)
    with pytest.raises(ValueError):
        S.measure(Acq(), (None, 86016))
    with pytest.raises(ValueError):
        S.measure(Acq(), (None, T.TWO_BLOCKS), source='track')


# ---------------------------------------------------------------- tools/run_file.py
def test_save_ephemeris_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_file
    _, info = T.strong()
    table = {}
    for prn, e in info['ephs'].items():               # as a run holds them: numpy scalars, the SAT key
        table[prn] = {k: (np.float64(v) if isinstance(v, float) else np.int64(v)) for k, v in e.items()}
        table[prn]['SAT'] = prn
    path = str(tmp_path / 'gpsEphem.json')
    run_file.save_ephemerides(path, table)
    back = run_file.load_ephemerides(path)
    keys = S.P.EPHEM_SF1 + S.P.EPHEM_SF2 + S.P.EPHEM_SF3
    assert sorted(back) == sorted(info['ephs'])
    for prn, e in info['ephs'].items():
        assert set(back[prn]) == set(keys)
        assert all(back[prn][k] == e[k] and type(back[prn][k]) is type(e[k]) for k in keys)
    m, ref = truth_fix()
    fx = S.coarse_time_fix(m, back, T.t_gps_of(info, MID), T.TRUTH)
    assert fx.ok and np.array_equal(fx.ecef, ref.ecef)


def test_decoded_ephemerides_of_a_solver(tmp_path):
    """What run() hands to --save-ephemeris: the tables of a PositionSolver that has read
    subframes 1-3 of two satellites and only subframe 1 of a third."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_file
    from gpsmi import navbits
    _, info = T.strong()
    solver = S.P.PositionSolver()
    for prn, sids in ((2, (1, 2, 3)), (5, (1, 2, 3)), (8, (1,))):
        for sid in sids:
            _, f = navbits.encode_nav_subframe(sid, 50001, info['ephs'][prn])
            solver.orbit(prn).read_frame(dict(f, SAT=prn, ST=65536 * sid))
    got = run_file.decoded_ephemerides(solver)
    assert sorted(got) == [2, 5]
    path = str(tmp_path / 'gpsEphem.json')
    run_file.save_ephemerides(path, got)
    back = run_file.load_ephemerides(path)
    keys = S.P.EPHEM_SF1 + S.P.EPHEM_SF2 + S.P.EPHEM_SF3
    assert back == {prn: {k: info['ephs'][prn][k] for k in keys} for prn in (2, 5)}


def test_time_argument():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_file
    _, info = T.strong()
    assert run_file.parse_time('299999.82', info['ephs']) == 299999.82
    # week 290 + 2 * 1024 starts 2024-10-27 00:00:00 GPS = 2024-10-26 23:59:42 UTC
    assert run_file.parse_time('2024-10-26T23:59:42', info['ephs']) == 0.0
    assert run_file.parse_time('2024-10-30T11:19:41Z', info['ephs']) == 3 * 86400 + 11 * 3600 + 19 * 60 + 59.0


def test_largest_peak_among_the_bins_that_detect():
    """pipeline.largest_peak_hits with corr_min: a weak PRN's largest peak is a strong satellite's
    cross-correlation in another bin (normMaxCorr below the threshold there); an absent PRN has no
    hit; without corr_min the rule is the one WeakAssist has always used."""
    from gpsmi._lib import PEAK_DTYPE
    from gpsmi.pipeline import largest_peak_hits
    tab = np.zeros((3, 3), PEAK_DTYPE)                # [bins, PRNs 4 (strong), 3 (weak), 27 (absent)]
    tab['mean'], tab['std'] = 10.0, 1.0
    tab['peak'] = [[60.0, 16.4, 14.0], [300.0, 15.5, 15.0], [80.0, 15.1, 13.0]]
    tab['std'][:, 1] = [1.0, 0.2, 0.5]                # the weak PRN: normMaxCorr 6.4, 27.5, 10.2
    tab['argmax'] = [[7, 494, 1], [8, 1380, 2], [9, 1381, 3]]

    class Engine:
        def search_deep(self, data, prns, freqs, n_coh, n_seg, f_offset=0.0):
            return tab

    class Acq:
        engine = Engine()
    freqs = [-1600.0, 3000.0, 3200.0]
    plain = largest_peak_hits(Acq(), None, [4, 3, 27], freqs)
    assert [(s, f, d) for _, s, f, d in plain] == [(4, 3000.0, 8), (3, -1600.0, 494), (27, 3000.0, 2)]
    hits = largest_peak_hits(Acq(), None, [4, 3, 27], freqs, corr_min=8.0)
    assert [(s, f, d) for _, s, f, d in hits] == [(4, 3000.0, 8), (3, 3000.0, 1380)]
    assert abs(hits[1][0] - 27.5) < 1e-4
