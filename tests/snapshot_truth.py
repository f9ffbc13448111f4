"""Truth of a synth_nav.geometric_scene for the snapshot-fix tests: what gpsmi.snapshot.measure
would return for a perfect receiver at any stream sample (code phase from the scene's pos_poly,
Doppler from its derivative), the GPS time of that sample, and the scenes the CPU and GPU tests
share."""
import functools

import numpy as np

from gpsmi import position as P, synth_nav
from gpsmi.snapshot import MEAS_DTYPE
from weaknav_truth import arrival, doppler_at

TRUTH = np.array(P.geo_to_ecef(49.082961, 8.307581, 160.0))       # the README's position
LOWERED_AMP = 0.0046 * 10.0 ** (9.5 / 20.0)                       # 0.01373: 35.0 dB-Hz (wtrk_ref.STRONG_AMP)
STRONG_SECONDS, MIXED_SECONDS = 1.0, 1.2
MIXED_WEAK = (3, 7, 12)
TWO_BLOCKS = 131072
# (fix error in m, geometry factor g) of the float64 restatement chain with no a-priori position and
# the time 20 s off, per (scene, samples or None = all, source): tests/test_snapshot.py measures and
# asserts them, tests/test_gpu_snapshot.py forms its bounds from them.  The chain is independent of
# the GPU path for the three kernels only: the records are formed by the same host code
# (snapshot.refined_records / tracked_records) and solved by the same coarse_time_fix, which have
# the truth measurements of this file as their own check
REF = {('strong', None, 'refine'): (17.62, 1.906), ('strong', None, 'track'): (7.69, 1.906),
       ('mixed', None, 'refine'): (1116.2, 22.95), ('mixed', None, 'track'): (419.6, 22.94),
       ('strong', TWO_BLOCKS, 'refine'): (10.98, 1.906)}


def truth_meas(scene, sample, mid=None, cn0=45.0, prns=None):
    """MEAS_DTYPE records of every satellite of `scene` (or of `prns`) as of stream index
    `sample`: the first code start at or behind it, the Doppler at stream index `mid` (default
    `sample`)."""
    cs = scene.code_samples
    sats = [s for s in scene.sats if prns is None or s.prn in prns]
    out = np.zeros(len(sats), MEAS_DTYPE)
    for r, s in zip(out, sorted(sats, key=lambda s: s.prn)):
        coefs, k0, ks = s.pos_poly
        m = np.ceil(np.polyval(coefs, (float(sample) - k0) / ks) / cs)
        k = float(arrival(s, m, cs))
        if k < sample:                                # (rounding at an exact code start)
            k = float(arrival(s, m + 1, cs))
        r['prn'], r['sample'], r['code_phase'] = s.prn, int(sample), k - sample
        r['f_hz'] = float(doppler_at(s, sample if mid is None else mid))
        r['cn0_dbhz'], r['edge'], r['source'] = cn0, np.nan, b'truth'
    return out


def phase_error(scene, meas):
    """Measured minus true code phase of every record, samples, folded into +-cs / 2."""
    cs = scene.code_samples
    err = np.zeros(len(meas))
    for i, r in enumerate(meas):
        t = truth_meas(scene, int(r['sample']), prns=[int(r['prn'])])[0]
        err[i] = (r['code_phase'] - t['code_phase'] + cs / 2.0) % cs - cs / 2.0
    return err


def edge_error(scene, meas):
    """`edge` of every record minus the nearest true bit edge (the arrival of a code period that
    is a multiple of 20), samples."""
    cs = scene.code_samples
    err = np.zeros(len(meas))
    for i, r in enumerate(meas):
        sat = next(s for s in scene.sats if s.prn == r['prn'])
        edges = arrival(sat, 20.0 * np.arange(-100, 200), cs)
        err[i] = r['edge'] - edges[np.argmin(np.abs(edges - r['edge']))]
    return err


def doppler_error(scene, meas, mid):
    t = truth_meas(scene, 0, mid=mid, prns=[int(p) for p in meas['prn']])
    return meas['f_hz'] - t['f_hz']


def t_gps_of(info, sample, fs=2048000.0):
    return info['t0_gps'] + sample / fs


@functools.lru_cache(maxsize=None)
def strong():
    """The 1-s strong scene: eight satellites, PRNs 2/5/8/10/13/16/19/21, default amplitude."""
    return synth_nav.geometric_scene(TRUTH, STRONG_SECONDS, n_sats=8, seed=79)


@functools.lru_cache(maxsize=None)
def mixed():
    """The 1.2-s mixed scene: six satellites, PRNs 3/7/12 lowered to 35 dB-Hz."""
    sc, info = synth_nav.geometric_scene(TRUTH, MIXED_SECONDS, n_sats=6, lead_s=0.25, seed=89)
    for s in sc.sats:
        if s.prn in MIXED_WEAK:
            s.amp = LOWERED_AMP
    return sc, info


@functools.lru_cache(maxsize=None)
def raw(name):
    """The recorder's uint16 samples of a scene, read-only: 'strong', 'mixed'."""
    sc, _ = {'strong': strong, 'mixed': mixed}[name]()
    n = int(round({'strong': STRONG_SECONDS, 'mixed': MIXED_SECONDS}[name] * 1000)) * sc.code_samples
    out = sc.block_raw(0, n=n)
    out.setflags(write=False)
    return out


def c64(name):
    from gpsmi.synth import raw_to_c64
    return raw_to_c64(raw(name))
