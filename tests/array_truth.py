"""The scene of the array search: the strong snapshot scene's eight satellites
(snapshot_truth.strong: PRNs 2/5/8/10/13/16/19/21, one second at 2.048 Msps) seen by four antennas
through a steering matrix of seeded unit phases (no line array), no jammer, every satellite at AMP --
too weak for the deep search of one antenna, within reach of the four together.

AMP was chosen on the float64 restatement (tests/array_ref.py), restricted to each satellite's three
nearest bins and a handful of empty cells; test_acq_array_scene.py holds the conditions:
  - antenna 0's deep search leaves at least four of the eight below corr_min - 1, the array's T puts
    all eight above corr_min + 1 at the true lag;
  - the largest normMaxCorr over absent PRNs stays below corr_min - 1 for both.
The same scene rendered 6 dB stronger (10 log10 4 = 6.0 dB is what four coherent antennas can give)
and measured on antenna 0 alone is the reference of the GPU test."""
import functools

import numpy as np

import acq_ref as ar
import array_ref as R
import snapshot_truth as T
from deep_ref import DEEP_AMP, deep_bins

ANTENNAS = 4
N_COH, N_SEG = 4, 250
SECONDS = 1.0
START_AMP = DEEP_AMP * 10.0 ** (-5.0 / 20.0)         # 0.002587: about 20.5 dB-Hz at sigma 0.35
AMP = START_AMP
STEER_SEED = 7919
CORR_MIN = 8.0
ABSENT = (4, 27)                                      # PRNs that are not in the scene
REFERENCE_DB = 20.0 * np.log10(2.0)                   # the amplitude doubled: 6.02 dB


def steering():
    """complex [4][8]: a unit phase per antenna and satellite, seeded."""
    rng = np.random.default_rng(STEER_SEED)
    return np.exp(2j * np.pi * rng.random((ANTENNAS, 8)))


@functools.lru_cache(maxsize=None)
def scene(gain_db=0.0):
    """(ArrayScene, info) with every satellite at AMP scaled by gain_db."""
    from gpsmi import synth_array, synth_nav
    sc, info = synth_nav.geometric_scene(T.TRUTH, SECONDS, n_sats=8, seed=79, amp=AMP * 10.0 ** (gain_db / 20.0))
    return synth_array.ArrayScene(sc, steering()), info


@functools.lru_cache(maxsize=None)
def raw(gain_db=0.0):
    """uint16 [4][2048000], read-only."""
    out = np.ascontiguousarray(scene(gain_db)[0].block_raw(0, n=int(SECONDS * 1000) * 2048))
    out.setflags(write=False)
    return out


def true_lags(sc):
    """{prn: (Doppler at sample 0, code start at or behind sample 0 as the searches report it)}"""
    return {int(r['prn']): (float(r['f_hz']), float(r['code_phase'])) for r in T.truth_meas(sc, 0)}


def z_at(S, lag=None):
    """(normMaxCorr of a surface, its argmax), or z at `lag` +- 1."""
    mean, std = np.mean(S), np.std(S)
    if lag is None:
        return (S.max() - mean) / std, int(np.argmax(S))
    k = int(np.rint(lag))
    return max((S[(k + d) % len(S)] - mean) / std for d in (-1, 0, 1))


@functools.lru_cache(maxsize=None)
def restated(gain_db=0.0):
    """The float64 restatement on the scene, per satellite over its three nearest bins and for the
    ABSENT PRNs over the bins of the first two satellites: {prn: dict(z0 = antenna 0's deep
    normMaxCorr (the largest of the bins), zT = the array's, zT_true = the array's z at the true lag
    +- 1 in the nearest bin, lag0 / lagT = the argmaxes there, lag = the true one)} and the absent
    PRNs' largest (z0, zT)."""
    sc = scene(gain_db)[0].scene
    rows = [ar.decode_u8(r) for r in raw(gain_db)]
    truth = true_lags(sc)
    out, absent = {}, [0.0, 0.0]
    for i, (prn, (dop, lag)) in enumerate(sorted(truth.items())):
        bins = deep_bins(dop)
        m = ar.deep_shifts(bins, N_COH, N_SEG, 2048)
        best = dict(z0=-np.inf, zT=-np.inf, lag=lag)
        for b, f in enumerate(bins):
            c = R.correlations(rows, f, [prn] + (list(ABSENT) if i < 2 else []), N_COH, N_SEG, m[b])
            S0, Tt = np.mean(np.abs(c[prn][0]), axis=0), R.combine(c[prn])
            (z0, l0), (zT, lT) = z_at(S0), z_at(Tt)
            if b == 1:                                 # the nearest bin
                best.update(zT_true=z_at(Tt, lag), z0_true=z_at(S0, lag), lag0=l0, lagT=lT)
            best['z0'], best['zT'] = max(best['z0'], z0), max(best['zT'], zT)
            for p in ABSENT if i < 2 else ():
                absent[0] = max(absent[0], z_at(np.mean(np.abs(c[p][0]), axis=0))[0])
                absent[1] = max(absent[1], z_at(R.combine(c[p]))[0])
        out[prn] = best
    return out, tuple(absent)
