"""Numpy restatement of the deep search (gpsmi_acq_search_deep) and the pinned deep scene, shared
by test_acq_deep.py (CPU) and test_gpu_acq_deep.py (GPU).

Semantics (include/gpsmi.h): segment s of bin b is the non-coherent search's segment; its
magnitude row is rotated by the integer code-Doppler shift
    m[b][s] = rint(-(f_b - f_offset) / carrier_hz * s * n_coh * cs)        (float64, half to even)
before it is added: S[i] = (1 / n_seg) sum_s |corr_s[(i + m[b][s]) mod cs]|."""
import numpy as np

import gps_oracle as orc

L1_HZ = 1575.42e6

# ---- the deep scene: one second at 2.048 Msps.  Four weak satellites at |Doppler| >= 4 kHz (both
# signs) whose code slides 5.3 .. 6.3 samples over the second, one weak satellite near 0 Hz that
# does not move.  Integer code delays at the start of the data, Dopplers within 40 Hz of a
# 200-Hz bin.  C/N0 = amp^2 fs / sigma^2: 25.5 dB-Hz at amp 0.0046, sigma 0.35 and 2.048 Msps.
DEEP_AMP = 0.0046
DEEP_HIGH = [(6, -4830.0, 412.0), (15, -4170.0, 1650.0), (23, 4230.0, 957.0), (29, 4810.0, 1311.0)]
DEEP_ZERO = (10, 30.0, 705.0)
DEEP_SEED = 41
DEEP_N_COH, DEEP_N_SEG = 4, 250


def deep_scene(code_samples=2048, n_cyc=32, amp=DEEP_AMP):
    """Scene of the DEEP satellites with synth's default delay_rate = -doppler / 1575.42e6 (the
    delays scaled to the code length)."""
    from gpsmi import synth
    k = code_samples / 2048.0
    sats = [synth.Sat(prn=p, doppler=f, delay=float(np.floor(d * k)), amp=amp,
                      phase0=0.7 * i) for i, (p, f, d) in enumerate(DEEP_HIGH + [DEEP_ZERO])]
    return synth.Scene(sats=sats, seed=DEEP_SEED, noise_sigma=0.35,
                       code_samples=code_samples, n_cyc=n_cyc)


def nearest_bin(f, step=200.0):
    return round(f / step) * step


def deep_bins(doppler, step=200.0):
    """A satellite's nearest bin and its two neighbours."""
    c = nearest_bin(doppler, step)
    return [c - step, c, c + step]


def deep_shifts(freqs, n_coh, n_seg, cs, carrier_hz=L1_HZ, f_offset=0.0):
    """m[b][s], int64 [nbins, n_seg] (not reduced mod cs)."""
    f = np.asarray(freqs, np.float64)[:, None]
    s = np.arange(n_seg, dtype=np.float64)[None, :]
    return np.rint(-(f - f_offset) / carrier_hz * s * n_coh * cs).astype(np.int64)


def deep_table(data, freqs, prns, n_coh, n_seg, p, carrier_hz=L1_HZ, f_offset=0.0):
    """nc_table (test_acq_noncoherent.py) with each segment's magnitude row rotated by m before it
    is added: the oracle's demod_doppler / folded_spectrum / circ_corr / peak_stats, the same sum
    order and scale.  Returns its dict of [nbins, nsv] arrays, 'second' included."""
    cs = p.code_samples
    t = orc.sec_time(p)
    spectra = {s: orc.fft_cacode(s, cs) for s in prns}
    nb, ns = len(freqs), len(prns)
    out = dict(argmax=np.zeros((nb, ns), np.int32), peak=np.zeros((nb, ns)),
               mean=np.zeros((nb, ns)), std=np.zeros((nb, ns)), second=np.zeros((nb, ns)))
    span = n_coh * cs
    scale = np.float32(1.0 / n_seg)
    m = deep_shifts(freqs, n_coh, n_seg, cs, carrier_hz, f_offset)
    for b, f in enumerate(freqs):
        acc = [np.zeros(cs, np.float32) for _ in prns]
        for g in range(n_seg):
            wiped, _ = orc.demod_doppler(data[g * span:(g + 1) * span], f, 0, span, t)
            spec = orc.folded_spectrum(wiped, 0, n_coh, cs)
            for j, s in enumerate(prns):
                corr = orc.circ_corr(spec, spectra[s])
                if m[b, g] % cs:
                    corr = np.roll(corr, -int(m[b, g]))       # corr[(i + m) mod cs] at i
                acc[j] = acc[j] + corr
        for j in range(ns):
            surf = acc[j] * scale
            mx, peak, mean, std = orc.peak_stats(surf)
            out['second'][b, j] = np.partition(surf, cs - 2)[cs - 2]
            out['argmax'][b, j] = mx
            out['peak'][b, j] = peak
            out['mean'][b, j] = mean
            out['std'][b, j] = std
    return out
