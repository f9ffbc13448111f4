"""The scenes of tests/test_gpu_weaknav.py, synthesised once per session.

Mixed scene: geometric_scene(truth, 9.6 s, n_sats=6, lead_s=2.0, seed=89); the three satellites with the
largest |Doppler| (seed 89: 3094 / 1698 / 2393 Hz) are lowered to the amplitude of the weak tracker's "strong" scene
(wtrk_ref.STRONG_AMP, amp^2 fs / sigma^2 = 35.0 dB-Hz), the other three keep the default.  Timing:
the receiver's cold sweep takes 25 blocks (0.8 s), the deep search the 32 blocks behind it (to
1.82 s); the weak channels start at 0.8 s and have their bits right from bit 20 on (1.2 s), so
with lead_s = 2.0 the first whole subframe starts arriving 0.8 s later than that, at 2.07 .. 2.09
s, and ends at 8.09 s; the scene ends 1.5 s = 75 bits behind it.
Picking the seed (CPU): 77, synth_nav's default, has a PDOP of 7.4 over its six satellites and the
oracle's 1-ms receiver loses the third of its strong ones (935 Hz); 89 has 3.8 and strong Dopplers
of 277 / -276 / -585 Hz.  With 89 the oracle's acq_table, 4 ms, on the two bins each of the 25 sweep
blocks visits gives the lowered PRNs 3 / 7 / 12 at most normMaxCorr 6.76 / 5.39 / 5.52; CORR_MIN is 8
(DESIGN.md 4.2h)."""
import functools

import numpy as np

from gpsmi import position as P, synth_nav

TRUTH = np.array(P.geo_to_ecef(49.082961, 8.307581, 160.0))
LOWERED_AMP = 0.0046 * 10.0 ** (9.5 / 20.0)      # wtrk_ref.STRONG_AMP
MIXED_BLOCKS, MIXED_LEAD, MIXED_SEED = 300, 2.0, 89
ONE_BLOCKS = 282                                  # test 2: 9.02 s


@functools.lru_cache(maxsize=None)
def mixed():
    """-> (scene, info, lowered PRNs)."""
    sc, info = synth_nav.geometric_scene(TRUTH, MIXED_BLOCKS * 0.032, n_sats=6, lead_s=MIXED_LEAD, seed=MIXED_SEED)
    order = sorted(sc.sats, key=lambda s: -abs(s.doppler))
    for s in order[:3]:
        s.amp = LOWERED_AMP
    return sc, info, sorted(s.prn for s in order[:3])


@functools.lru_cache(maxsize=None)
def mixed_blocks():
    sc, _, _ = mixed()
    out = [sc.block(b) for b in range(MIXED_BLOCKS)]
    for b in out:
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def one():
    """Test 2: the default amplitude, four satellites, the same lead."""
    return synth_nav.geometric_scene(TRUTH, ONE_BLOCKS * 0.032, n_sats=4, lead_s=MIXED_LEAD)


@functools.lru_cache(maxsize=None)
def one_blocks():
    sc, _ = one()
    out = [sc.block(b) for b in range(ONE_BLOCKS)]
    for b in out:
        b.setflags(write=False)
    return out
