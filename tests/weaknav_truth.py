"""Truth of a synth_nav.geometric_scene for the weak-channel hand-off tests: when every code
start arrives (the scene's pos_poly inverted), and the bit records a perfect tracker would return."""
import numpy as np

from gpsmi._lib import WTRK_BIT_DTYPE
from gpsmi.synth_nav import F_L1


def arrival(sat, period, cs):
    """Stream position (samples, float64) at which code period `period` (array) of `sat` starts:
    pos(k) = period * cs solved by Newton; pos' is 1 + doppler / L1, so four steps are plenty."""
    coefs, k0, ks = sat.pos_poly
    d1 = np.polyder(coefs)
    target = np.asarray(period, dtype=np.float64) * cs
    k = target - np.polyval(coefs, (0.0 - k0) / ks)
    for _ in range(6):
        x = (k - k0) / ks
        k = k - (np.polyval(coefs, x) - target) / (np.polyval(d1, x) / ks)
    return k


def doppler_at(sat, k):
    """The Doppler the code slides with at stream position k: (d pos / d k - 1) * L1."""
    coefs, k0, ks = sat.pos_poly
    return (np.polyval(np.polyder(coefs), (np.asarray(k) - k0) / ks) / ks - 1.0) * F_L1


def truth_records(sat, cs, b0, n_samples, amp=100.0, b_end=None):
    """WTRK_BIT_DTYPE records of `sat` from bit b0 on, every bit that ends inside n_samples (or up
    to b_end): p_i = +-amp from nav_bits, tau the arrival of the bit's first code start, f_hz the
    Doppler there, bit_no counting from 0."""
    if b_end is None:
        b = np.arange(b0, b0 + int(n_samples // (20 * cs)) + 2)
        b = b[arrival(sat, 20 * (b + 1), cs) <= n_samples]
    else:
        b = np.arange(b0, b_end)
    rec = np.zeros(len(b), WTRK_BIT_DTYPE)
    nav = np.asarray(sat.nav_bits)
    rec['tau'] = arrival(sat, 20 * b, cs)
    rec['f_hz'] = doppler_at(sat, rec['tau'])
    rec['p_i'] = amp * (2.0 * nav[b % len(nav)] - 1.0)
    rec['cn0_dbhz'], rec['lock'] = 45.0, 1.0
    rec['bit_no'] = np.arange(len(b))
    return rec, b
