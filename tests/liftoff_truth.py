"""The lift-off scene of the correlation-profile tests, shared by test_profile.py
(CPU) and test_gpu_snapshot_profile.py (GPU): snapshot_truth's strong scene with every satellite
doubled by synth_nav.add_spoofer from LIFT_OFF_M east of the truth, LIFT_CLOCK_S late and LIFT_GAIN_DB
stronger -- a spoofer that has just started to drag: every copy lies within a chip or so of the
authentic code, inside the guard of the auxiliary peaks, so no PRN is doubled."""
import functools

import numpy as np

import snapshot_truth as T
from gpsmi import snapshot as S, synth_nav

LIFT_OFF_M, LIFT_CLOCK_S, LIFT_GAIN_DB = 150.0, 0.5e-6, 3.0
# the PRNs the restated chain (restated() below, then profile_ref and snapshot.profile_verdict) flags as
# distorted: tests/test_profile.py measures and asserts them, tests/test_gpu_snapshot_profile.py and
# tests/test_run_file_profile.py hold the GPU path to them (as spoof_truth.REF)
REF_DISTORTED = [5, 16, 19, 21]


def spoofer_pos():
    east, _, _ = S.enu_axes(T.TRUTH)
    return T.TRUTH + LIFT_OFF_M * east


@functools.lru_cache(maxsize=None)
def liftoff():
    """(scene, info, the Sats added): a scene of its own (snapshot_truth.strong() is shared)."""
    sc, info = synth_nav.geometric_scene(T.TRUTH, T.STRONG_SECONDS, n_sats=8, seed=79)
    added = synth_nav.add_spoofer(sc, info, spoofer_pos(), clock_s=LIFT_CLOCK_S, gain_db=LIFT_GAIN_DB)
    return sc, info, added


@functools.lru_cache(maxsize=None)
def raw():
    sc = liftoff()[0]
    out = sc.block_raw(0, n=int(round(T.STRONG_SECONDS * 1000)) * sc.code_samples)
    out.setflags(write=False)
    return out


def copy_offsets():
    """Per PRN the copy's code start behind the authentic one at sample 0, in samples (signed)."""
    sc, _, added = liftoff()
    cs = sc.code_samples
    out = {}
    for b in added:
        a = next(s for s in sc.sats if s.prn == b.prn and s is not b)
        lag = [(-np.polyval(s.pos_poly[0], (0.0 - s.pos_poly[1]) / s.pos_poly[2])) % cs for s in (a, b)]
        out[b.prn] = float((lag[1] - lag[0] + cs / 2.0) % cs - cs / 2.0)
    return out


@functools.lru_cache(maxsize=None)
def restated():
    """-> (records MEAS_DTYPE, SpoofReport) of the restated chain of test_snapshot_spoof.py (restated deep
    rows -> peaks_ref -> refine_ref over +- one bin step, re-centred -> snapshot.spoof_keep, source
    'refine') on the lift-off scene, the search restricted to the true PRNs and their bins."""
    import collective_ref as CR
    import gps_oracle as orc
    import peaks_ref as R
    from deep_ref import deep_bins
    from gpsmi.pipeline import hits_of_picks
    from gpsmi.synth import raw_to_c64
    from refine_ref import refine_ref
    from test_snapshot_spoof import BIN_STEP, CORR_MIN
    sc = liftoff()[0]
    data = raw_to_c64(raw())
    cs, n = sc.code_samples, len(data)
    n_seg = n // cs // 4
    found = []
    for prn in sorted({s.prn for s in sc.sats}):
        bins = deep_bins(float(T.truth_meas(T.strong()[0], 0, mid=n // 2, prns=[prn])['f_hz'][0]))
        rows = CR.deep_rows(data[:n_seg * 4 * cs], bins, [prn], 4, n_seg, orc.Params())
        picks, cols = R.peaks(rows, S.SPOOF_PICKS)
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
    return out, report
