"""The scenes of the spoofing-check tests, shared by test_snapshot_spoof.py (CPU)
and test_gpu_snapshot_spoof.py (GPU): snapshot_truth's strong scene (eight satellites, 1 s) and the
same scene with every satellite doubled by synth_nav.add_spoofer -- a spoofer that replays what a
receiver SPOOF_OFF_M north of the truth would see, SPOOF_CLOCK_S late and SPOOF_GAIN_DB stronger."""
import functools

import numpy as np

import snapshot_truth as T
from gpsmi import snapshot as S, synth_nav

SPOOF_OFF_M, SPOOF_CLOCK_S, SPOOF_GAIN_DB = 2.0e3, 30.0e-6, 3.0
APRIORI_OFF_M, TIME_OFF = 5.0e3, 20.0        # the a-priori: 5 km east of the truth, the time 20 s off
# (fix error in m, geometry factor g) of the two fixes of the float64 restatement chain (restated
# deep rows -> peaks_ref -> refine_ref -> spoof_keep -> twin_fixes, source 'refine') on the spoofed
# scene, each against its own position: tests/test_snapshot_spoof.py measures and asserts them,
# tests/test_gpu_snapshot_spoof.py forms its bounds from them (as snapshot_truth.REF)
REF = {'truth': (42.91, 2.263), 'spoofer': (31.11, 2.263)}


def spoofer_pos():
    _, north, _ = S.enu_axes(T.TRUTH)
    return T.TRUTH + SPOOF_OFF_M * north


def apriori():
    east, _, _ = S.enu_axes(T.TRUTH)
    return T.TRUTH + APRIORI_OFF_M * east


@functools.lru_cache(maxsize=None)
def spoofed():
    """(scene, info, the Sats added): a scene of its own (snapshot_truth.strong() is shared)."""
    sc, info = synth_nav.geometric_scene(T.TRUTH, T.STRONG_SECONDS, n_sats=8, seed=79)
    added = synth_nav.add_spoofer(sc, info, spoofer_pos(), clock_s=SPOOF_CLOCK_S, gain_db=SPOOF_GAIN_DB)
    return sc, info, added


@functools.lru_cache(maxsize=None)
def raw():
    sc = spoofed()[0]
    out = sc.block_raw(0, n=int(round(T.STRONG_SECONDS * 1000)) * sc.code_samples)
    out.setflags(write=False)
    return out


def pair_spacing():
    """Per PRN the circular distance in lags between the two copies' code starts at sample 0."""
    sc, _, added = spoofed()
    cs = sc.code_samples
    out = {}
    for b in added:
        a = next(s for s in sc.sats if s.prn == b.prn and s is not b)
        lag = [(-np.polyval(s.pos_poly[0], (0.0 - s.pos_poly[1]) / s.pos_poly[2])) % cs for s in (a, b)]
        d = abs(lag[0] - lag[1])
        out[b.prn] = min(d, cs - d)
    return out
