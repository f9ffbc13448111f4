"""The spoofing check with several antennas without a GPU: the restated chain of
test_snapshot_spoof.py on antenna 0 -- the records are its records -- then the float64 restatement of
the signatures (sig_ref.py) over four antennas and the host decision the GPU path uses
(snapshot.signature_vectors, spoof_resolve).  The scenes are spoof_truth.py's through
synth_array.ArrayScene: a uniform line of four antennas, the eight authentic satellites at the sines
-0.875 + 0.25 i, everything the spoofer sends at the sine 0.3.  The signatures are taken over the
first sig_ref.SIG_MS milliseconds."""
import numpy as np

import sig_ref as R
import snapshot_truth as T
import spoof_truth as ST
import test_snapshot_spoof as TS
from gpsmi import snapshot as S
from gpsmi.synth import raw_to_c64

CS = 2048
N_SIG = (R.SIG_MS + 2) * CS


def signatures(which, meas):
    """-> (v, quality) of the records `meas` over the first SIG_MS milliseconds of the scene."""
    rows = raw_to_c64(R.snapshot_raw(which, R.SIG_MS + 2))
    sats = [(int(r['prn']), float(r['f_hz']), float(r['sample'] + r['code_phase'])) for r in meas]
    _, cov, n_win = R.sig_ref(rows, sats, CS, n_ms=R.SIG_MS)
    assert n_win.tolist() == [R.SIG_MS] * len(meas)
    return S.signature_vectors(cov)


def added_lags():
    """Per PRN the code start at sample 0 of the signal the spoofer added (spoof_truth.pair_spacing's rule)."""
    return {b.prn: (-np.polyval(b.pos_poly[0], (0.0 - b.pos_poly[1]) / b.pos_poly[2])) % CS for b in ST.spoofed()[2]}


def is_added(rec):
    d = abs(rec['code_phase'] - added_lags()[int(rec['prn'])])
    return min(d, CS - d) < 1.0


def test_antenna_0_is_the_single_antenna_scene():
    for which, raw in (('spoofed', ST.raw()), ('clean', T.raw('strong'))):
        rows = R.snapshot_raw(which, R.SIG_MS + 2)
        assert rows.shape == (R.SNAP_ANTENNAS, N_SIG) and np.array_equal(rows[0], raw[:N_SIG])
        assert not np.array_equal(rows[1], rows[0])


def test_spoofed_scene_verdict():
    _, info, _ = ST.spoofed()
    meas, report, _ = TS.restated(True)
    report = S.SpoofReport(doubled=list(report.doubled), alarm=report.alarm)      # (restated's is shared)
    assert len(meas) == 16 and report.doubled == sorted(info['ephs'])
    v, quality = signatures('spoofed', meas)
    rho = S.signature_rho(v)
    spoofer = [i for i, r in enumerate(meas) if is_added(r)]
    authentic = [i for i in range(len(meas)) if i not in spoofer]
    assert len(spoofer) == 8 and sorted(meas['prn'][spoofer].tolist()) == sorted(info['ephs'])
    same = min(rho[i, j] for k, i in enumerate(spoofer) for j in spoofer[k + 1:])
    auth_least = min(rho[i, j] for k, i in enumerate(authentic) for j in authentic[k + 1:])
    auth_most = max(rho[i, j] for k, i in enumerate(authentic) for j in authentic[k + 1:])
    steer = R.snapshot_array('spoofed').steering
    to_truth = min(abs(np.vdot(steer[:, 8] / 2.0, v[i])) for i in spoofer)
    print('same-source pairs: least rho %.4f; authentic pairs: least %.4f, largest %.4f; spoofer signatures within '
          '%.4f of the steering vector; quality %.1f .. %.1f' % (same, auth_least, auth_most, to_truth, quality.min(),
                                                                 quality.max()))
    assert same >= S.SPOOF_RHO_MIN
    assert auth_least < S.SPOOF_RHO_MIN
    # whatever the a-priori says: near the truth the authentic fix comes first from twin_fixes, near
    # the spoofer the spoofer's does; the verdict names the authentic one both times
    for pos, first in ((ST.apriori(), 'truth'), (ST.spoofer_pos() + 100.0, 'spoofer')):
        rep = S.SpoofReport(doubled=list(report.doubled), alarm=report.alarm)
        S.twin_fixes(meas, info['ephs'], info['t0_gps'] + ST.TIME_OFF, pos, rep)
        assert rep.fixes[1] is not None and rep.sets is not None
        near = {'truth': T.TRUTH, 'spoofer': ST.spoofer_pos()}[first]
        assert np.linalg.norm(rep.fixes[0].ecef - near) < 200.0
        auth = S.spoof_resolve(rep, meas, rep.sets, v)
        assert auth == (0 if first == 'truth' else 1) and rep.authentic == auth and not rep.one_direction
        assert rep.one_source == ((False, True) if auth == 0 else (True, False))
        # the spoofer's set holds the code phases of the Sats that were added, the authentic one none
        # (the pair of least rms holds one PRN the wrong way round, which either fix drops: seven records each)
        print('   sets', rep.sets, 'dropped', [f.dropped for f in rep.fixes])
        assert set(rep.sets[1 - auth]) <= set(spoofer) and set(rep.sets[auth]) <= set(authentic)
        assert min(len(ix) for ix in rep.sets) >= 7
        fix = rep.fixes[auth]
        assert S.authentic_first(rep) is fix and rep.fixes[0] is fix and rep.authentic == 0     # snapshot_fix's order
        assert rep.one_source == (False, True) and set(rep.sets[1]) <= set(spoofer)
        err = np.linalg.norm(fix.ecef - T.TRUTH)
        print('a-priori near the %s: authentic = fixes[%d], %.2f m from the truth' % (first, auth, err))
        assert fix.ok and abs(err - ST.REF['truth'][0]) <= 0.05 * ST.REF['truth'][0]


def test_clean_scene_raises_nothing():
    """Without the spoofer: the records are the single-antenna chain's (antenna 0 is its input), no
    doubled PRN, no verdict, no alarm."""
    meas, report, _ = TS.restated(False)
    before = meas.tobytes()
    report = S.SpoofReport(doubled=list(report.doubled), alarm=report.alarm)
    v, quality = signatures('clean', meas)
    assert S.spoof_resolve(report, meas, None, v) is None
    rho = S.signature_rho(v)
    off = rho[~np.eye(len(meas), dtype=bool)]
    print('clean scene: rho of the pairs %.4f .. %.4f' % (off.min(), off.max()))
    assert report.doubled == [] and not report.alarm and not report.one_direction and report.authentic is None
    assert off.min() < S.SPOOF_RHO_MIN and meas.tobytes() == before


def test_spoofer_alone_is_one_direction():
    """The authentic amplitudes 0 -- a spoofer that has swamped the sky: no PRN is doubled, the
    twin check sees nothing, and every record arrives from one direction."""
    import collective_ref as CR
    import gps_oracle as orc
    import peaks_ref as PR
    from deep_ref import deep_bins
    from gpsmi.pipeline import hits_of_picks
    from refine_ref import refine_ref
    n = T.TWO_BLOCKS
    rows = raw_to_c64(R.snapshot_raw('spoofer', R.SIG_MS + 2))
    data = rows[0][:n]
    n_seg = n // CS // 4
    found = []
    for prn in sorted({s.prn for s in ST.spoofed()[0].sats}):
        bins = deep_bins(float(T.truth_meas(T.strong()[0], 0, mid=n // 2, prns=[prn])['f_hz'][0]))
        picks, cols = PR.peaks(CR.deep_rows(data[:n_seg * 4 * CS], bins, [prn], 4, n_seg, orc.Params()), S.SPOOF_PICKS)
        found += hits_of_picks(picks, cols, [prn], bins, TS.CORR_MIN)
    n_ms = ((n - 1) // CS - 2) // 20 * 20
    rec = refine_ref(data, [h[1:] for h in found], n_ms, CS, df_half=TS.BIN_STEP)[0]
    rec, found, meas, report = S.spoof_keep(rec, found, CS)
    # (64 ms do not confirm every one of the eight; SPOOF_DIRECTION_PRNS records are what the rule needs)
    print('spoofer alone: PRNs', meas['prn'].tolist())
    assert report.doubled == [] and not report.alarm and all(is_added(r) for r in meas)
    assert len(set(meas['prn'].tolist())) == len(meas) >= S.SPOOF_DIRECTION_PRNS
    _, cov, n_win = R.sig_ref(rows, [(int(r['prn']), float(r['f_hz']), float(r['code_phase'])) for r in meas], CS,
                              n_ms=R.SIG_MS)
    v, _ = S.signature_vectors(cov)
    assert S.spoof_resolve(report, meas, None, v) is None
    off = report.rho[~np.eye(len(meas), dtype=bool)]
    print('spoofer alone: least rho %.4f' % off.min())
    assert off.min() >= S.SPOOF_RHO_MIN and report.one_direction and report.alarm and report.doubled == []
