"""Non-coherent acquisition (gpsmi_acq_search_nc), the parts that need no GPU: the ABI
declarations, a numpy restatement of the search built from the oracle's own steps, and the
weak-signal scene the GPU tests (test_gpu_acq_noncoherent.py) detect on.

Semantics (include/gpsmi.h): segment s of a search covers code periods [s n_coh, (s+1) n_coh)
and is the reference's coherent search (gpsrecv.py:249-259) on the samples from there on, the
carrier wipe-off restarting at phase 0; the surface is (1/n_seg) sum_s |corr_s| in float32."""
import ctypes as C
import os
import re

import numpy as np

import gps_oracle as orc
from conftest import ROOT, scene_blocks

HEADER = os.path.join(ROOT, 'include', 'gpsmi.h')

# ---- the weak scene: four SVs at amp 0.010 (C/N0 = amp^2 fs / sigma^2, about 32 dB-Hz at
# 2.048 Msps and sigma 0.35), integer code delays, Dopplers within 40 Hz of a 200-Hz bin
WEAK_AMP = 0.010
WEAK = [(5, -2960.0, 311.0), (12, -1030.0, 1101.0), (19, 780.0, 1703.0), (27, 2420.0, 905.0)]
ABSENT = [3, 8, 22, 30]
WEAK_SEED = 23


def weak_scene(code_samples=2048, n_cyc=32, strong=()):
    """Scene of the WEAK satellites (delays scaled to the code length), plus `strong`
    (prn, doppler, delay) ones at the default amplitude 0.06."""
    from gpsmi import synth
    k = code_samples / 2048.0
    sats = [synth.Sat(prn=p, doppler=f, delay=float(np.floor(d * k)), amp=WEAK_AMP,
                      phase0=0.7 * i) for i, (p, f, d) in enumerate(WEAK)]
    sats += [synth.Sat(prn=p, doppler=f, delay=float(np.floor(d * k)), phase0=1.3)
             for p, f, d in strong]
    return synth.Scene(sats=sats, seed=WEAK_SEED, noise_sigma=0.35,
                       code_samples=code_samples, n_cyc=n_cyc)


def nearest_bin(f, step=200.0):
    return round(f / step) * step


def nc_table(data, freqs, prns, n_coh, n_seg, p):
    """Restatement of gpsmi_acq_search_nc with the oracle's demod_doppler / folded_spectrum /
    circ_corr / peak_stats: per bin and segment the coherent surface of acq_table, the
    magnitudes summed in float32 in ascending segment order and scaled by float32(1 / n_seg).
    Returns acq_table's dict of [nbins, nsv] arrays, plus 'second': the surface's second
    largest value (where it is within 1e-4 of the peak, the argmax may fall on either)."""
    cs = p.code_samples
    t = orc.sec_time(p)
    spectra = {s: orc.fft_cacode(s, cs) for s in prns}
    nb, ns = len(freqs), len(prns)
    out = dict(argmax=np.zeros((nb, ns), np.int32), peak=np.zeros((nb, ns)),
               mean=np.zeros((nb, ns)), std=np.zeros((nb, ns)), second=np.zeros((nb, ns)))
    span = n_coh * cs
    scale = np.float32(1.0 / n_seg)
    for b, f in enumerate(freqs):
        acc = [np.zeros(cs, np.float32) for _ in prns]
        for g in range(n_seg):
            wiped, _ = orc.demod_doppler(data[g * span:(g + 1) * span], f, 0, span, t)
            spec = orc.folded_spectrum(wiped, 0, n_coh, cs)
            for j, s in enumerate(prns):
                acc[j] = acc[j] + orc.circ_corr(spec, spectra[s])
        for j in range(ns):
            surf = acc[j] * scale
            mx, peak, mean, std = orc.peak_stats(surf)
            out['second'][b, j] = np.partition(surf, cs - 2)[cs - 2]
            out['argmax'][b, j] = mx
            out['peak'][b, j] = peak
            out['mean'][b, j] = mean
            out['std'][b, j] = std
    return out


def nmc_of(tab):
    return (tab['peak'] - tab['mean']) / tab['std']


# ---- ABI ---------------------------------------------------------------------------------

def test_header_declares_noncoherent_search():
    src = open(HEADER).read()
    for name, nargs in (('gpsmi_acq_search_nc', 11), ('gpsmi_acq_search_nc_dev', 11)):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} not declared'
        assert len(m.group(1).split(',')) == nargs
    from gpsmi import _lib
    lib = _lib.load()
    for name in ('gpsmi_acq_search_nc', 'gpsmi_acq_search_nc_dev'):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def test_null_handle_is_an_argument_error():
    from gpsmi import _lib
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    prn = np.array([1], np.int32)
    f = np.array([0.0])
    out = np.zeros(1, _lib.PEAK_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.gpsmi_acq_search_nc(None, p(buf), 8, p(prn), 1, p(f), 1, 1, 1, p(out), None) == -1
    assert lib.gpsmi_acq_search_nc_dev(None, p(buf), 8, p(prn), 1, p(f), 1, 1, 1, p(out),
                                       None) == -1
    assert b'null' in lib.gpsmi_last_error()


# ---- the restatement ----------------------------------------------------------------------

def test_restatement_with_one_segment_is_acq_table():
    """n_seg = 1: 0 + m = m and m * 1 = m, so nc_table is the oracle's coherent table to the
    bit on the default fixture scene."""
    data = scene_blocks('default', 0, 1)[0]
    p = orc.Params()
    freqs = [-5000.0 + 200 * i for i in range(0, 51, 5)]
    prns = list(range(2, 33, 3))
    for n_coh in (1, 4):
        ref = orc.acq_table(data, freqs, prns, n_coh, p)
        got = nc_table(data, freqs, prns, n_coh, 1, p)
        for k in ('argmax', 'peak', 'mean', 'std'):
            assert np.array_equal(got[k], ref[k]), (n_coh, k)


def test_weak_scene_needs_noncoherent_integration():
    """The pinned weak scene: every weak SV is lost in the reference's 4-ms search (< 6) and
    stands out at 25 x 4 ms (>= 10, argmax within 1 of the true delay); absent PRNs stay < 6
    at 25 x 4 ms (and below CORR_MIN in the 4-ms search, whose noise peaks spread wider)."""
    sc = weak_scene()
    p = orc.Params()
    data = sc.block(0, n=25 * 4 * 2048)
    freqs = [nearest_bin(f) for _, f, _ in WEAK]
    prns = [s for s, _, _ in WEAK] + ABSENT
    coh = orc.acq_table(data, freqs, prns, 4, p)
    nc = nc_table(data, freqs, prns, 4, 25, p)
    for b, (prn, _, delay) in enumerate(WEAK):
        assert nmc_of(coh)[b, b] < 6, (prn, nmc_of(coh)[b, b])
        assert nmc_of(nc)[b, b] >= 10, (prn, nmc_of(nc)[b, b])
        assert abs(int(nc['argmax'][b, b]) - int(delay)) <= 1, (prn, nc['argmax'][b, b])
    na = len(WEAK)
    assert np.all(nmc_of(coh)[:, na:] < p.corr_min)
    assert np.all(nmc_of(nc)[:, na:] < 6), nmc_of(nc)[:, na:]
