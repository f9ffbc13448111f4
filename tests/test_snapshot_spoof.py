"""The spoofing check without a GPU: the restated chain -- restated deep rows
(collective_ref.deep_rows) -> peaks_ref -> pipeline.hits_of_picks -> refine_ref over +- one bin step
with refine_centred's re-centring -> snapshot.spoof_keep -> snapshot.twin_fixes -- on the strong
scene with and without a spoofer (spoof_truth.py).  As in test_snapshot.py the search is restricted
to the true PRNs and their bins +- 1, and the records are formed and solved by the host code the GPU
path uses."""
import functools

import numpy as np
import pytest

import collective_ref as CR
import peaks_ref as R
import snapshot_truth as T
import spoof_truth as ST
from gpsmi import snapshot as S

FS = 2048000.0
CORR_MIN = 8.0
BIN_STEP = 200.0


@functools.lru_cache(maxsize=None)
def restated(spoofed):
    """-> (records MEAS_DTYPE, SpoofReport, picks per PRN) of the restated chain, source 'refine'."""
    import gps_oracle as orc
    from deep_ref import deep_bins
    from gpsmi.pipeline import hits_of_picks
    from gpsmi.synth import raw_to_c64
    from refine_ref import refine_ref
    sc = ST.spoofed()[0] if spoofed else T.strong()[0]
    data = raw_to_c64(ST.raw()) if spoofed else T.c64('strong')
    cs, n = sc.code_samples, len(data)
    n_seg = n // cs // 4
    found, picks_of = [], {}
    for prn in sorted({s.prn for s in sc.sats}):
        bins = deep_bins(float(T.truth_meas(T.strong()[0], 0, mid=n // 2, prns=[prn])['f_hz'][0]))
        rows = CR.deep_rows(data[:n_seg * 4 * cs], bins, [prn], 4, n_seg, orc.Params())
        picks, cols = R.peaks(rows, S.SPOOF_PICKS)
        picks_of[prn] = picks[0]
        found += hits_of_picks(picks, cols, [prn], bins, CORR_MIN)
    n_ms = ((n - 1) // cs - 2) // 20 * 20
    rec = refine_ref(data, [h[1:] for h in found], n_ms, cs, df_half=BIN_STEP)[0]
    for _ in range(2):
        bad = [i for i, r in enumerate(rec) if r['confirmed'] == 1 and r['code_phase'] < 0]
        for i in bad:
            z, s, f, d = found[i]
            e, _, l = rec[i]['tap_metric']
            found[i] = (z, s, f, int(d + (-1 if e > l else 1)) % cs)
        if bad:
            rec[bad] = refine_ref(data, [found[i][1:] for i in bad], n_ms, cs, df_half=BIN_STEP)[0]
    rec, found, out, report = S.spoof_keep(rec, found, cs)
    return out, report, picks_of


def test_pairs_are_apart():
    """Every pair three guards apart or more (the picks must resolve them with room to spare) and
    none wider than the contract's largest guard, half a code period."""
    sp = ST.pair_spacing()
    print('pair spacing in lags:', {p: round(d, 1) for p, d in sp.items()})
    assert len(sp) == 8
    assert min(sp.values()) >= 3 * R.default_guard(2048) and max(sp.values()) <= 2048 // 2


def test_add_spoofer():
    sc, info, added = ST.spoofed()
    own = sc.sats[:8]
    assert [s.prn for s in added] == [s.prn for s in own] and len(sc.sats) == 16
    for a, b in zip(own, added):
        assert b.nav_bits is a.nav_bits and b.amp == pytest.approx(a.amp * 10.0 ** (ST.SPOOF_GAIN_DB / 20.0))
        assert abs(b.doppler - a.doppler) < 5.0            # 2 km move a Doppler by a few Hz at the most
    # the added signals are those of a receiver at the spoofer's position whose clock is late
    m = T.truth_meas(type(sc)(sats=added, code_samples=sc.code_samples), 0)
    t_gps = info['t0_gps'] - ST.SPOOF_CLOCK_S
    fx = S.coarse_time_fix(m, info['ephs'], t_gps, ST.apriori())
    assert fx.ok and np.linalg.norm(fx.ecef - ST.spoofer_pos()) < 1.0


def test_spoofed_scene_twin_fixes():
    _, info, _ = ST.spoofed()
    meas, report, picks = restated(True)
    for prn, pk in picks.items():
        print(prn, [(int(k['lag']), round(float(k['z']), 1)) for k in pk])
    assert report.doubled == sorted(info['ephs']) and len(report.doubled) == 8 and report.alarm
    assert meas['prn'].tolist() == sorted(2 * sorted(info['ephs'])) and not report.crowded
    fix = S.twin_fixes(meas, info['ephs'], info['t0_gps'] + ST.TIME_OFF, ST.apriori(), report)
    fa, fb = report.fixes
    assert fix is fa and fa.ok and fb.ok, (fa.reason, fb.reason)
    assert report.assignments == 128
    err = {'truth': np.linalg.norm(fa.ecef - T.TRUTH), 'spoofer': np.linalg.norm(fb.ecef - ST.spoofer_pos())}
    print('fix_a %.2f m from the truth (g %.3f, rms %.1f m), fix_b %.2f m from the spoofer (g %.3f, rms %.1f m), '
          'separation %.1f m' % (err['truth'], fa.g, fa.rms_m, err['spoofer'], fb.g, fb.rms_m, report.separation_m))
    assert abs(report.separation_m - ST.SPOOF_OFF_M) < 100.0
    for which, fx in (('truth', fa), ('spoofer', fb)):
        print('   %s: %d satellites, dropped %s' % (which, len(fx.prns), fx.dropped))
        assert abs(err[which] - ST.REF[which][0]) <= 0.05 * ST.REF[which][0]
        assert abs(fx.g - ST.REF[which][1]) <= 0.01 * ST.REF[which][1]


def test_clean_scene_is_todays():
    """Without the spoofer: no doubled PRN, no alarm, and the records and the Fix of today's chain
    (test_snapshot.py's restatement, one hit per PRN, refinement over +- 120 Hz)."""
    from test_snapshot import restated as today
    _, info = T.strong()
    meas, report, _ = restated(False)
    assert report.doubled == [] and not report.alarm and not report.crowded
    ref = today('strong')['refine']
    assert meas.tobytes() == ref.tobytes()
    assert S.twin_sets(meas) == [(list(range(8)), list(range(8)))]
    fix = S.twin_fixes(meas, info['ephs'], info['t0_gps'] + ST.TIME_OFF, ST.apriori(), report)
    r = int(np.argmax(S.cn0_weights(ref['cn0_dbhz'])))
    want = S.coarse_time_fix(ref, info['ephs'], info['t0_gps'] + ST.TIME_OFF + ref['sample'][r] / FS, ST.apriori())
    assert fix.ok and report.fixes[1] is None and report.separation_m is None
    assert np.array_equal(fix.ecef, want.ecef) and fix.t_gps == want.t_gps and fix.prns == want.prns
    assert np.array_equal(fix.residuals, want.residuals)


def test_keep_rule():
    from gpsmi._lib import REFINE_OUT_DTYPE
    rec = np.zeros(7, REFINE_OUT_DTYPE)
    rec['prn'] = [4, 4, 4, 9, 9, 11, 4]
    rec['confirmed'], rec['code_phase'], rec['n_bits'] = 1, [10.5, 80.2, 300.0, 5.0, 700.0, 40.0, 900.0], 48
    rec['f_hz'] = [1000.0, 1003.0, 1040.0, -2300.0, -2330.0, 300.0, 1002.0]     # (nobody is anybody's ghost)
    rec['cn0_dbhz'] = [45.0, 48.0, 32.0, 50.0, 37.9, 44.0, 40.0]
    assert not S.drop_ghosts(rec).any()
    found = [(20.0, int(p), 0.0, int(c)) for p, c in zip(rec['prn'], rec['code_phase'])]
    kept, f, out, rep = S.spoof_keep(rec, found, 2048)
    # PRN 4: 48, 45 and 40 are within 12 dB of 48 (crowded: the two strongest stay), 32 is not;
    # PRN 9: 37.9 is 12.1 dB under 50
    assert out['prn'].tolist() == [4, 4, 9, 11] and out['cn0_dbhz'].tolist() == [45.0, 48.0, 50.0, 44.0]
    assert rep.doubled == [4] and rep.crowded and not rep.alarm
    assert S.spoof_keep(rec, found, 2048, min_doubled=1)[3].alarm
    assert S.twin_sets(out) == [([0, 2, 3], [1, 2, 3])]


def test_twin_sets_enumeration():
    m = np.zeros(7, S.MEAS_DTYPE)
    m['prn'], m['cn0_dbhz'] = [2, 2, 5, 8, 8, 9, 9], [40, 43, 45, 41, 44, 39, 42]
    sets = S.twin_sets(m)
    assert len(sets) == 4 and len({(tuple(a), tuple(b)) for a, b in sets}) == 4
    for a, b in sets:
        assert 2 in a and 2 in b and 0 in a and 1 in b         # the single record in both, the first pair fixed
        assert sorted(a + b) == [0, 1, 2, 2, 3, 4, 5, 6] and len(a) == len(b) == 4
