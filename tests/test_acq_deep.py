"""Deep acquisition (gpsmi_acq_search_deep), the parts that need no GPU: the ABI declarations,
the numpy restatement deep_table (deep_ref.py) against nc_table where nothing shifts, and the
pinned deep scene the GPU tests (test_gpu_acq_deep.py) detect on.

Semantics (include/gpsmi.h): the non-coherent search with every segment's magnitude row rotated
by m[b][s] = rint(-(f_b - f_offset) / carrier_hz * s * n_coh * cs) before it is added, so that a
satellite's peak stays on its code phase at the start of the data over spans of seconds."""
import ctypes as C
import os
import re

import numpy as np

import gps_oracle as orc
from conftest import ROOT, scene_blocks
from deep_ref import (DEEP_HIGH, DEEP_N_COH, DEEP_N_SEG, DEEP_ZERO, L1_HZ, deep_bins, deep_scene,
                      deep_shifts, deep_table, nearest_bin)
from test_acq_noncoherent import nc_table, nmc_of

HEADER = os.path.join(ROOT, 'include', 'gpsmi.h')

# The guard bands of the detection statement, from the numpy restatement on the pinned scene
# (test_deep_scene_needs_code_doppler_compensation's docstring has the measured values): the
# uncompensated search comes within 0.66 of CORR_MIN = 8 from below, the deep search stays 2.25
# above it; each assertion keeps at most half of that distance as its guard band.
NC_BELOW = 8 - 0.33
DEEP_ABOVE = 8 + 1.12


# ---- ABI ---------------------------------------------------------------------------------

def test_header_declares_deep_search():
    src = open(HEADER).read()
    for name in ('gpsmi_acq_search_deep', 'gpsmi_acq_search_deep_dev'):
        m = re.search(r'int\s+' + name + r'\s*\(([^)]*)\)', src)
        assert m, f'{name} not declared'
        args = [a.strip() for a in m.group(1).split(',')]
        assert len(args) == 13
        assert args[9] == 'double carrier_hz' and args[10] == 'double f_offset_hz'
    from gpsmi import _lib
    lib = _lib.load()
    for name in ('gpsmi_acq_search_deep', 'gpsmi_acq_search_deep_dev'):
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
    assert lib.gpsmi_acq_search_deep(None, p(buf), 8, p(prn), 1, p(f), 1, 1, 1, L1_HZ, 0.0,
                                     p(out), None) == -1
    assert lib.gpsmi_acq_search_deep_dev(None, p(buf), 8, p(prn), 1, p(f), 1, 1, 1, L1_HZ, 0.0,
                                         p(out), None) == -1
    assert b'null' in lib.gpsmi_last_error()


# ---- the restatement ----------------------------------------------------------------------

def test_shift_table():
    """Sign, size and rounding of m: a satellite at +f slides to earlier lags (synth's delay_rate
    is -f / carrier), 1.3 samples per second and kHz at 2.048 Msps; ties go to the even integer."""
    m = deep_shifts([-5000.0, 0.0, 5000.0], 4, 250, 2048)
    assert m.shape == (3, 250) and np.all(m[:, 0] == 0) and np.all(m[1] == 0)
    assert m[0, 249] == 6 and m[2, 249] == -6                    # 6.47 samples after 0.996 s
    assert np.array_equal(m[0], -m[2]) and np.all(np.diff(m[0]) >= 0)
    # f_offset: the bin frequency minus the offset is the Doppler that moves the code
    assert np.array_equal(deep_shifts([5000.0], 4, 250, 2048, f_offset=5000.0), np.zeros((1, 250)))
    # exact halves: with f = -carrier / 4096 and cs = 2048 the slide is 0.5 sample per segment
    tie = deep_shifts([-L1_HZ / 4096.0], 1, 6, 2048)
    assert tie.tolist() == [[0, 0, 1, 2, 2, 2]]                   # 0, .5, 1, 1.5, 2, 2.5 -> half to even


def test_restatement_without_shift_is_nc_table():
    """Where every m is 0 -- 100 ms at 2.048 Msps slide 0.65 samples at 5 kHz, the rounding
    reaches 1 only beyond 3.8 kHz; here |f| <= 3 kHz -- deep_table is nc_table to the bit."""
    data = np.concatenate(scene_blocks('default', 0, 2))[:10 * 4 * 2048]
    p = orc.Params()
    freqs = [-3000.0 + 600.0 * i for i in range(11)]
    prns = list(range(2, 33, 5))
    assert not deep_shifts(freqs, 4, 10, 2048).any()
    ref = nc_table(data, freqs, prns, 4, 10, p)
    got = deep_table(data, freqs, prns, 4, 10, p)
    for k in ('argmax', 'peak', 'mean', 'std', 'second'):
        assert np.array_equal(got[k], ref[k]), k
    # a large f_offset that cancels the bin: again no shift, again the same bits
    got = deep_table(data, [4000.0], prns, 4, 10, p, f_offset=4000.0)
    ref = nc_table(data, [4000.0], prns, 4, 10, p)
    for k in ('argmax', 'peak', 'mean', 'std', 'second'):
        assert np.array_equal(got[k], ref[k]), k


def test_deep_scene_needs_code_doppler_compensation():
    """The pinned deep scene (deep_ref.py): 1 s (250 x 4 ms) at 2.048 Msps, amplitude 0.0046
    (25.5 dB-Hz), four satellites at -4830 / -4170 / +4230 / +4810 Hz whose code slides 5.3 .. 6.3
    samples over the span, one at +30 Hz that stays.  Bins: each satellite's nearest 200-Hz bin
    +- 1 (the whole test: about 8 s on one core).  Measured with the restatement, normMaxCorr at
    the nearest bin:

        PRN   Doppler    nc_table (argmax)   deep_table (argmax)   true delay
          6   -4830 Hz    4.28  (417)          10.99 (412)            412
         15   -4170 Hz    5.22  (1651)         10.25 (1650)          1650
         23   +4230 Hz    5.87  (954)          10.45 (957)            957
         29   +4810 Hz    7.34  (1306)         13.29 (1311)          1311
         10     +30 Hz   12.98  (705)          12.98 (705)            705

    Neighbouring bins stay at 2.9 .. 4.0 in both.  The uncompensated search is 0.66 below
    CORR_MIN = 8 at its closest, the deep search 2.25 above it: asserted with guard bands of
    0.33 and 1.12."""
    sc = deep_scene()
    p = orc.Params()
    data = sc.block(0, n=DEEP_N_SEG * DEEP_N_COH * 2048)
    for prn, dop, delay in DEEP_HIGH:
        bins = deep_bins(dop)
        nc = nmc_of(nc_table(data, bins, [prn], DEEP_N_COH, DEEP_N_SEG, p))[:, 0]
        tab = deep_table(data, bins, [prn], DEEP_N_COH, DEEP_N_SEG, p)
        dp = nmc_of(tab)[:, 0]
        print(prn, dop, 'nc', nc, 'deep', dp, tab['argmax'][:, 0])
        assert np.all(nc < NC_BELOW), (prn, nc)
        assert dp[1] > DEEP_ABOVE, (prn, dp)
        assert abs(int(tab['argmax'][1, 0]) - int(delay)) <= 1, (prn, tab['argmax'][:, 0])
        assert dp[0] < NC_BELOW and dp[2] < NC_BELOW, (prn, dp)
    prn, dop, delay = DEEP_ZERO
    bins = [nearest_bin(dop)]
    nc = nc_table(data, bins, [prn], DEEP_N_COH, DEEP_N_SEG, p)
    tab = deep_table(data, bins, [prn], DEEP_N_COH, DEEP_N_SEG, p)
    print(prn, dop, 'nc', nmc_of(nc), 'deep', nmc_of(tab))
    for t in (nc, tab):
        assert nmc_of(t)[0, 0] > DEEP_ABOVE
        assert abs(int(t['argmax'][0, 0]) - int(delay)) <= 1
