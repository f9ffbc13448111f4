"""GPU: the deep search (gpsmi_acq_search_deep / AcqEngine.search_deep / Acquisition.sweepDeepSats)
against the non-coherent search where nothing shifts (bytewise), against the numpy restatement
deep_table (deep_ref.py) where it does, and on the deep scene it exists for.  The bars against the
restatement are test_gpu_acq_noncoherent.py's (_check_restated)."""
import numpy as np
import pytest

import gps_oracle as orc
from deep_ref import (DEEP_HIGH, DEEP_N_COH, DEEP_N_SEG, DEEP_ZERO, deep_bins, deep_scene,
                      deep_shifts, deep_table, nearest_bin)
from test_acq_deep import DEEP_ABOVE, NC_BELOW
from test_acq_noncoherent import nmc_of
from test_gpu_acq_noncoherent import CFG, _check_restated, _engine, _same, _upload

pytestmark = pytest.mark.gpu

GRID = [-5000.0 + 200.0 * i for i in range(51)]


def _params(cs):
    return orc.Params(code_samples=cs, n_cyc=CFG[cs]['n_cyc'])


@pytest.fixture(scope='module')
def deep_data():
    """The pinned deep scene, 1 s (250 x 4 ms) at 2.048 Msps, raw and complex64."""
    from gpsmi.synth import raw_to_c64
    raw = deep_scene().block_raw(0, n=DEEP_N_SEG * DEEP_N_COH * 2048)
    return raw, raw_to_c64(raw)


# ---- 1. where every shift is 0 the records are the non-coherent search's, byte for byte ----

@pytest.mark.parametrize('cs, n_coh, n_seg', [(2048, 4, 6), (16368, 2, 3)])
@pytest.mark.parametrize('raw', [False, True])
def test_span_too_short_to_slide_equals_noncoherent(cs, n_coh, n_seg, raw):
    """The whole +-5 kHz bin list over 24 ms (2048) / 6 ms (16368): the slide stays under half a
    sample, every m is 0.  Host and device-resident input, neighbours included."""
    from gpsmi.synth import raw_to_c64
    n = n_seg * n_coh * cs
    data = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.05).block_raw(0, n=n)
    if not raw:
        data = raw_to_c64(data)
    prns = [6, 15, 23, 29, 10, 3]
    assert not deep_shifts(GRID, n_coh, n_seg, cs).any()
    e = _engine(cs, raw)
    try:
        ref, ref_nbr = e.search_noncoherent(data, prns, GRID, n_coh, n_seg, nbr=True)
        got, nbr = e.search_deep(data, prns, GRID, n_coh, n_seg, nbr=True)
        _same(got, ref)
        _same(nbr, ref_nbr)
        buf = _upload(data)
        try:
            _same(e.search_deep((buf.ptr, n), prns, GRID, n_coh, n_seg), ref)
        finally:
            buf.free()
    finally:
        e.close()


@pytest.mark.parametrize('raw', [False, True])
def test_zero_hz_bin_over_one_second_equals_noncoherent(deep_data, raw):
    """A 0 Hz bin never shifts, however long the span; nor does a bin that f_offset cancels."""
    data = deep_data[0] if raw else deep_data[1]
    prns = [10, 6, 29, 3]
    e = _engine(2048, raw)
    try:
        ref = e.search_noncoherent(data, prns, [0.0], DEEP_N_COH, DEEP_N_SEG)
        _same(e.search_deep(data, prns, [0.0], DEEP_N_COH, DEEP_N_SEG), ref)
        ref = e.search_noncoherent(data, prns, [4800.0], DEEP_N_COH, DEEP_N_SEG)
        _same(e.search_deep(data, prns, [4800.0], DEEP_N_COH, DEEP_N_SEG, f_offset=4800.0), ref)
        # ... and the same bin without the offset does shift: other bytes
        got = e.search_deep(data, prns, [4800.0], DEEP_N_COH, DEEP_N_SEG)
        assert got.tobytes() != ref.tobytes()
    finally:
        e.close()


@pytest.mark.parametrize('cs, n_seg', [(2048, 1000), (16368, 250), (16368, 1000)])
@pytest.mark.parametrize('raw', [False, True])
def test_seconds_from_device_input(cs, n_seg, raw):
    """n_coh 4 x 250 (1 s) and x 1000 (4 s) segments from device-resident input (100 ms of a
    scene, repeated): the call works, and its 0 Hz bin is the non-coherent search's byte for
    byte.  (1 s at 2048 is the deep scene of the tests around this one.)"""
    from gpsmi.engine import DeviceBuffer
    from gpsmi.synth import raw_to_c64
    n_coh = 4
    piece = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.02).block_raw(0, n=25 * n_coh * cs)
    if not raw:
        piece = raw_to_c64(piece)
    n = n_seg * n_coh * cs
    buf = DeviceBuffer(n * piece.itemsize)
    e = _engine(cs, raw)
    try:
        for k in range(n // piece.size):
            buf.upload(piece, k * piece.nbytes)
        prns = [10, 6]
        ref = e.search_noncoherent((buf.ptr, n), prns, [0.0], n_coh, n_seg)
        _same(e.search_deep((buf.ptr, n), prns, [0.0], n_coh, n_seg), ref)
        tab = e.search_deep((buf.ptr, n), prns, [0.0, 4800.0], n_coh, n_seg)
        _same(tab[:1], ref)
        assert e.last_ms() > 0
    finally:
        e.close()
        buf.free()


# ---- 2. against the restatement --------------------------------------------------------------

def test_restatement_deep_scene(deep_data):
    """Every deep-scene satellite's nearest bin +- 1, all five PRNs plus two absent ones, 250 x
    4 ms: shifts 0 .. +-6 samples."""
    data = deep_data[1]
    freqs = sorted({f for _, dop, _ in DEEP_HIGH + [DEEP_ZERO] for f in deep_bins(dop)})
    prns = [p for p, _, _ in DEEP_HIGH + [DEEP_ZERO]] + [3, 18]
    e = _engine(2048)
    try:
        tab = e.search_deep(data, prns, freqs, DEEP_N_COH, DEEP_N_SEG)
    finally:
        e.close()
    _check_restated(tab, deep_table(data, freqs, prns, DEEP_N_COH, DEEP_N_SEG, orc.Params()))


@pytest.mark.parametrize('cs', [2048, 16368])
@pytest.mark.parametrize('f_offset', [250e3, -250e3, 60e6])
def test_restatement_large_shifts(cs, f_offset):
    """A short span at a large f_offset_hz: shifts of several samples per segment in either
    direction (a negative m is a rotation by nearly the whole code length), and at 60 MHz
    hundreds (2048) to thousands (16368) of samples, across the rows of the 16368 layout."""
    n_coh, n_seg = 2, 5
    sc = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.05)
    data = sc.block(0, n=n_seg * n_coh * cs)
    prns = [6, 15, 23, 29, 10, 3]
    freqs = [-4800.0, -4200.0, 0.0, 4200.0, 4800.0]
    m = deep_shifts(freqs, n_coh, n_seg, cs, f_offset=f_offset)
    assert np.all(np.abs(m[:, 1:]) >= 1) and np.abs(m).max() >= (3 if abs(f_offset) < 1e6 else 600)
    e = _engine(cs)
    try:
        tab = e.search_deep(data, prns, freqs, n_coh, n_seg, f_offset=f_offset)
    finally:
        e.close()
    _check_restated(tab, deep_table(data, freqs, prns, n_coh, n_seg, _params(cs), f_offset=f_offset))


# ---- 3. detection on the deep scene ------------------------------------------------------------

def test_deep_scene_detection(deep_data):
    """sweepDeepSats over 31 SV x 51 bins finds every high-Doppler satellite at its bin and at
    the true delay +- 1; sweepWeakSats and search_noncoherent over the same second find none of
    them (and both find the 0 Hz one).  Guard bands as in test_acq_deep.py."""
    from gpsmi.acquisition import Acquisition
    data = deep_data[1]
    acq = Acquisition()
    try:
        sat_lst, found = list(range(2, 33)), []
        res = acq.sweepDeepSats(data, GRID, sat_lst, found, n_coh=DEEP_N_COH, n_seg=DEEP_N_SEG)
        assert res == sorted(found, reverse=True)
        got = {s: (f, d, nmc) for nmc, s, f, d in res}
        print('deep', res)
        for prn, dop, delay in DEEP_HIGH + [DEEP_ZERO]:
            assert prn in got, (prn, res)
            assert got[prn][0] == nearest_bin(dop)
            assert abs(got[prn][1] - int(delay)) <= 1
            assert got[prn][2] > DEEP_ABOVE
            assert prn not in sat_lst
        assert set(got) == {p for p, _, _ in DEEP_HIGH + [DEEP_ZERO]}
        lst2, found2 = list(range(2, 33)), []
        res2 = acq.sweepWeakSats(data, GRID, lst2, found2, n_coh=DEEP_N_COH, n_seg=DEEP_N_SEG)
        print('nc', res2)
        assert {s for _, s, _, _ in res2} == {DEEP_ZERO[0]}
        high = [p for p, _, _ in DEEP_HIGH]
        nc = nmc_of(acq.engine.search_noncoherent(data, high, GRID, DEEP_N_COH, DEEP_N_SEG))
        print('nc max per SV', nc.max(axis=0))
        assert np.all(nc < NC_BELOW)
    finally:
        acq.engine.close()


def test_run_file_deep_acq(tmp_path):
    """tools/run_file.py --deep-acq on the deep scene as a recording (32 whole blocks: the reader
    takes 32-ms blocks; the second pass uses the first second of them): the 4-ms sweep acquires
    nothing, the second pass reports the five satellites."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    path = tmp_path / 'deep.bin'
    deep_scene().block_raw(0, n=32 * 65536).tofile(path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), str(path),
                        '--seconds', '0.3', '--deep-acq', '1.0', '--json'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep['acquired'] == []
    d = rep['deep_acquisition']
    assert (d['n_coh'], d['n_seg']) == (DEEP_N_COH, DEEP_N_SEG) and d['device_ms'] > 0
    got = {s: (f, dly, nmc) for s, f, dly, nmc in d['found']}
    assert set(got) == {p for p, _, _ in DEEP_HIGH + [DEEP_ZERO]}
    for prn, dop, delay in DEEP_HIGH + [DEEP_ZERO]:
        assert got[prn][0] == nearest_bin(dop) and abs(got[prn][1] - int(delay)) <= 1


# ---- 4. the grouping of bins into a launch does not matter -------------------------------------

@pytest.mark.parametrize('cs, n_coh, n_seg, f_offset, widen', [(2048, 4, 250, 0.0, 1.0),
                                                              (16368, 2, 5, 3e6, 80.0)])
def test_all_bins_in_one_call_equal_per_bin_calls(deep_data, cs, n_coh, n_seg, f_offset, widen):
    """(At 16368 the span is 10 ms: the bins are spread over +-384 kHz so that each has shifts
    of its own; what the search finds there does not matter here.)"""
    if cs == 2048:
        data = deep_data[1]
    else:
        data = deep_scene(cs, 8, amp=0.05).block(0, n=n_seg * n_coh * cs)
    freqs = [widen * f for f in (-4800.0, 4800.0, 0.0, -4200.0, 2600.0, 4200.0)]
    prns = [6, 15, 23, 29, 10]
    m = deep_shifts(freqs, n_coh, n_seg, cs, f_offset=f_offset)
    assert len({tuple(r) for r in m}) == len(freqs)              # every bin its own shifts
    e = _engine(cs)
    try:
        whole, wn = e.search_deep(data, prns, freqs, n_coh, n_seg, f_offset=f_offset, nbr=True)
        for b, f in enumerate(freqs):
            one, on = e.search_deep(data, prns, [f], n_coh, n_seg, f_offset=f_offset, nbr=True)
            _same(one, whole[b:b + 1])
            _same(on, wn[b:b + 1])
        rev = e.search_deep(data, prns[::-1], freqs[::-1], n_coh, n_seg, f_offset=f_offset)
        _same(rev[::-1, ::-1], whole)
    finally:
        e.close()


# ---- 5. what is refused -------------------------------------------------------------------------

def test_other_code_length_is_unsupported():
    from gpsmi.engine import AcqEngine, Config, EngineError
    from gpsmi import synth
    e = AcqEngine(Config(code_samples=4096, n_cyc=8))
    try:
        data = synth.default_scene(4, seed=3, code_samples=4096, n_cyc=8).block(0)
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.search_deep(data, [3], [0.0], 2, 2)
        e.search(data, [3], [0.0], 2)
    finally:
        e.close()


@pytest.mark.parametrize('forced', [1, 2])
def test_time_domain_paths_are_unsupported(forced):
    from conftest import scene_blocks
    from gpsmi.engine import EngineError, clear_default, set_default
    set_default('codephase', forced)
    try:
        e = _engine(16368)
    finally:
        clear_default('codephase')
    try:
        data = scene_blocks('hirate', 0, 1)[0]
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.search_deep(data, [3], [0.0], 2, 2)
        e.search(data, [3], [0.0], 2)                    # the coherent search still runs
    finally:
        e.close()


@pytest.mark.parametrize('cs, n_seg_max', [(2048, 32768), (16368, 4100)])
def test_span_beyond_the_scratch_cap_is_unsupported(cs, n_seg_max):
    """One bin's segments must fit 512 MiB of scratch (n_seg * cs * 8 bytes: 32768 segments at
    2048, 4100 at 16368); one more is refused, host and device input, and the handle stays
    usable."""
    assert n_seg_max * cs * 8 <= 512 << 20 < (n_seg_max + 1) * cs * 8
    from gpsmi.engine import DeviceBuffer, EngineError
    n = (n_seg_max + 1) * cs
    e = _engine(cs, raw_u8=True)
    buf = DeviceBuffer(2 * n)                            # (raw samples; never read)
    try:
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.search_deep((buf.ptr, n), [3], [0.0], 1, n_seg_max + 1)
        host = np.zeros(n, np.uint16)
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.search_deep(host, [3], [0.0], 1, n_seg_max + 1)
        small = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.05).block_raw(0, n=4 * cs)
        _same(e.search_deep(small, [6, 3], [0.0, 4800.0], 2, 2),
              e.search_noncoherent(small, [6, 3], [0.0, 4800.0], 2, 2))
    finally:
        e.close()
        buf.free()


def test_argument_errors():
    from gpsmi.engine import EngineError
    e = _engine(2048)
    try:
        data = deep_scene(amp=0.05).block(0, n=2 * 2 * 2048)
        for kw in (dict(carrier_hz=0.0), dict(carrier_hz=-1.0), dict(carrier_hz=float('nan')),
                   dict(f_offset=float('inf'))):
            with pytest.raises(EngineError, match=r'\(-1\)'):
                e.search_deep(data, [3, 6], [0.0, 200.0], 2, 2, **kw)
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.search_deep(data, [3, 6], [0.0, float('nan')], 2, 2)
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.search_deep(data, [3, 6], [0.0, 200.0], 2, 3)          # iq too short
        tab = e.search_deep(data, [3, 6], [0.0, 200.0], 2, 2)
        _check_restated(tab, deep_table(data, [0.0, 200.0], [3, 6], 2, 2, orc.Params()))
    finally:
        e.close()
