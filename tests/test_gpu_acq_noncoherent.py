"""GPU: the non-coherent search (gpsmi_acq_search_nc / AcqEngine.search_noncoherent /
Acquisition.sweepWeakSats) against today's coherent search at one segment, against the numpy
restatement nc_table (test_acq_noncoherent.py) at many, and on the weak scene it exists for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gps_oracle as orc
from conftest import ROOT, scene_blocks, scene_for
from test_acq_noncoherent import (ABSENT, WEAK, nc_table, nearest_bin, nmc_of,
                                  weak_scene)

pytestmark = pytest.mark.gpu

RTOL = 1e-4
CFG = {2048: dict(code_samples=2048, n_cyc=32), 16368: dict(code_samples=16368, n_cyc=8)}
FIXTURE = {2048: 'default', 16368: 'hirate'}


def _engine(cs, raw_u8=False):
    from gpsmi.engine import AcqEngine, Config
    e = AcqEngine(Config(**CFG[cs]))
    if raw_u8:
        e.set_input_format(True)
    return e


@pytest.fixture(scope='module', params=[2048, 16368])
def eng(request):
    e = _engine(request.param)
    yield e
    e.close()


def _upload(arr):
    from gpsmi.engine import DeviceBuffer
    buf = DeviceBuffer(arr.nbytes)
    buf.upload(arr)
    return buf


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    assert np.array_equal(_bytes(a), _bytes(b))


def _check_restated(tab, ref):
    """The bars of the issue: peak / mean / std within rtol 1e-4; argmax exact where the top two
    lags of the restatement are apart by more than 1e-4 relative, else within one lag; no
    CORR_MIN flips except where normMaxCorr is within 1e-3 of it."""
    for k in ('peak', 'mean', 'std'):
        np.testing.assert_allclose(tab[k], ref[k], rtol=RTOL)
    tie = (ref['peak'] - ref['second']) <= 1e-4 * ref['peak']
    am, ram = tab['argmax'].astype(np.int64), ref['argmax'].astype(np.int64)
    assert np.array_equal(am[~tie], ram[~tie])
    assert np.all(np.abs(am[tie] - ram[tie]) <= 1)
    nmc = (tab['peak'].astype(np.float64) - tab['mean']) / tab['std']
    rn = nmc_of(ref)
    flip = (nmc > 8) != (rn > 8)
    assert np.all(np.abs(rn[flip] - 8) < 1e-3)


# ---- 1. one segment is today's search, bit for bit --------------------------------------

@pytest.mark.parametrize('cs, n_coh', [(2048, 1), (2048, 4), (2048, 10),
                                       (16368, 1), (16368, 4), (16368, 8)])
@pytest.mark.parametrize('raw', [False, True])
def test_one_segment_equals_coherent_search(cs, n_coh, raw):
    sc = scene_for(FIXTURE[cs])
    data = sc.block_raw(0) if raw else scene_blocks(FIXTURE[cs], 0, 1)[0]
    freqs = [-5000.0 + 250.0 * i for i in range(41)] if cs == 2048 else \
        [-4000.0 + 400.0 * i for i in range(21)]
    prns = list(range(1, 33)) if cs == 2048 else [s.prn for s in sc.sats][:8] + [1, 2]
    e = _engine(cs, raw)
    try:
        ref, ref_nbr = e.search_ex(data, prns, freqs, n_coh)
        _same(e.search(data, prns, freqs, n_coh), ref)
        got, nbr = e.search_noncoherent(data, prns, freqs, n_coh, 1, nbr=True)
        _same(got, ref)
        _same(nbr, ref_nbr)
        buf = _upload(data)
        try:
            _same(e.search_noncoherent((buf.ptr, data.size), prns, freqs, n_coh, 1), ref)
        finally:
            buf.free()
    finally:
        e.close()


# ---- 2. many segments match the restatement ----------------------------------------------

def test_restatement_2048_reference_grid():
    """31 SV x 51 bins (-5000 .. +5000 step 200) x n_coh 4 x n_seg 25, weak and strong SVs."""
    sc = weak_scene(strong=[(14, 1630.0, 77.0), (21, -420.0, 1500.0)])
    data = sc.block(0, n=25 * 4 * 2048)
    freqs = [-5000.0 + 200.0 * i for i in range(51)]
    prns = list(range(2, 33))
    e = _engine(2048)
    try:
        tab = e.search_noncoherent(data, prns, freqs, 4, 25)
    finally:
        e.close()
    _check_restated(tab, nc_table(data, freqs, prns, 4, 25, orc.Params()))


def test_restatement_16368():
    """8 SV x 11 bins x n_coh 2 x n_seg 5 on the 16.368-Msps fixture scene."""
    sc = scene_for('hirate')
    data = sc.block(0, n=5 * 2 * 16368)
    prns = [s.prn for s in sc.sats][:6] + [1, 2]
    freqs = [nearest_bin(sc.sats[0].doppler) + 200.0 * (i - 5) for i in range(11)]
    e = _engine(16368)
    try:
        tab = e.search_noncoherent(data, prns, freqs, 2, 5)
    finally:
        e.close()
    _check_restated(tab, nc_table(data, freqs, prns, 2, 5, orc.Params(code_samples=16368, n_cyc=8)))


# ---- 3. detection on the weak scene -------------------------------------------------------

def test_weak_scene_detection():
    from gpsmi.acquisition import Acquisition
    sc = weak_scene()
    data = sc.block(0, n=25 * 4 * 2048)
    acq = Acquisition()
    try:
        sat_lst = list(range(2, 33))
        found = []
        freqs = [-5000.0 + 200.0 * i for i in range(51)]
        res = acq.sweepWeakSats(data, freqs, sat_lst, found, n_coh=4, n_seg=25)
        assert res == sorted(found, reverse=True)
        got = {s: (f, d) for _, s, f, d in res}
        for prn, dop, delay in WEAK:
            assert prn in got, (prn, res)
            assert got[prn][0] == nearest_bin(dop)
            assert abs(got[prn][1] - int(delay)) <= 1
            assert prn not in sat_lst
        assert not set(got) & set(ABSENT)
        assert set(got) == {p for p, _, _ in WEAK}
        # the reference's own sweep over the same data finds none of them
        lst2, found2 = list(range(2, 33)), []
        _, _, res2 = acq.sweepAllSats(data[:32 * 2048], -5000.0, lst2, found2, itSweep=50)
        assert not {s for _, s, _, _ in res2} & {p for p, _, _ in WEAK}
    finally:
        acq.engine.close()


# ---- 4. input formats and device input at n_seg > 1 --------------------------------------

@pytest.mark.parametrize('cs, n_coh, n_seg', [(2048, 4, 6), (2048, 2, 5), (16368, 2, 3)])
def test_formats_and_device_input_agree(cs, n_coh, n_seg):
    sc = weak_scene(code_samples=cs, n_cyc=CFG[cs]['n_cyc'], strong=[(14, 1630.0, 77.0)])
    n = n_seg * n_coh * cs
    raw = sc.block_raw(0, n=n)
    from gpsmi.synth import raw_to_c64
    c64 = raw_to_c64(raw)
    freqs = [-1200.0 + 200.0 * i for i in range(14)]
    prns = [5, 12, 14, 19, 27, 3]
    ec, eu = _engine(cs), _engine(cs, raw_u8=True)
    try:
        ref, ref_nbr = ec.search_noncoherent(c64, prns, freqs, n_coh, n_seg, nbr=True)
        got, nbr = eu.search_noncoherent(raw, prns, freqs, n_coh, n_seg, nbr=True)
        _same(got, ref)
        _same(nbr, ref_nbr)
        bc, bu = _upload(c64), _upload(raw)
        try:
            _same(ec.search_noncoherent((bc.ptr, n), prns, freqs, n_coh, n_seg), ref)
            _same(eu.search_noncoherent((bu.ptr, n), prns, freqs, n_coh, n_seg), ref)
        finally:
            bc.free()
            bu.free()
    finally:
        ec.close()
        eu.close()


# ---- 5. full size -------------------------------------------------------------------------

@pytest.mark.parametrize('cs, nsv, nbins, n_coh, n_seg', [(2048, 31, 51, 4, 250),
                                                         (16368, 12, 21, 8, 25)])
def test_full_size(cs, nsv, nbins, n_coh, n_seg):
    """1 s at 2048 and 200 ms at 16368; a 4 SV x 3 bin subset against the restatement."""
    sc = weak_scene(code_samples=cs, n_cyc=CFG[cs]['n_cyc'], strong=[(13, 1630.0, 77.0)])
    data = sc.block(0, n=n_seg * n_coh * cs)
    prns = list(range(2, 2 + nsv))
    freqs = [-200.0 * (nbins // 2) + 200.0 * i for i in range(nbins)]
    e = _engine(cs)
    try:
        tab = e.search_noncoherent(data, prns, freqs, n_coh, n_seg)
        assert e.last_ms() > 0
    finally:
        e.close()
    sub_p = [5, 12, 13, 3]
    sub_f = [nearest_bin(-1030.0), nearest_bin(1630.0), 0.0]
    p = orc.Params(code_samples=cs, n_cyc=CFG[cs]['n_cyc'])
    ref = nc_table(data, sub_f, sub_p, n_coh, n_seg, p)
    bi = [freqs.index(f) for f in sub_f]
    si = [prns.index(s) for s in sub_p]
    _check_restated(tab[np.ix_(bi, si)], ref)


# ---- 6. errors ----------------------------------------------------------------------------

def test_argument_errors_leave_the_handle_usable(eng):
    from gpsmi.engine import EngineError
    cs, n_cyc = eng.cfg.code_samples, eng.cfg.n_cyc
    data = scene_for(FIXTURE[cs]).block(0, n=2 * 2 * cs)
    prns, freqs = [3, 5], [0.0, 200.0]
    for n_coh, n_seg, d in ((2, 0, data), (0, 2, data), (n_cyc + 1, 1, data),
                            (2, 2, data[:-1]), (2, 3, data)):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            eng.search_noncoherent(d, prns, freqs, n_coh, n_seg)
    tab = eng.search_noncoherent(data, prns, freqs, 2, 2)
    ref = nc_table(data, freqs, prns, 2, 2, orc.Params(code_samples=cs, n_cyc=n_cyc))
    _check_restated(tab, ref)


@pytest.mark.parametrize('forced', [1, 2])
def test_time_domain_paths_are_unsupported(forced):
    from gpsmi.engine import EngineError, clear_default, set_default
    set_default('codephase', forced)
    try:
        e = _engine(16368)
    finally:
        clear_default('codephase')
    try:
        data = scene_blocks('hirate', 0, 1)[0]
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.search_noncoherent(data, [3], [0.0], 2, 2)
        e.search(data, [3], [0.0], 2)                    # the coherent search still runs
    finally:
        e.close()


# ---- 7. the tool --------------------------------------------------------------------------

def test_acq_weak_tool(tmp_path):
    sc = weak_scene(strong=[(14, 1630.0, 77.0), (21, -420.0, 1500.0)])
    path = tmp_path / 'weak.bin'
    sc.block_raw(0, n=4 * 65536).tofile(path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'acq_weak.py'), str(path),
                        '--json'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    coh = {e['prn'] for e in rep['coherent'] if e['found']}
    weak = {e['prn'] for e in rep['weak'] if e['found']}
    assert {14, 21} <= coh and {14, 21} <= weak
    for prn, _, _ in WEAK:
        assert prn in weak and prn not in coh
    assert not (coh | weak) & set(ABSENT)
    assert rep['weak_ms'] > 0 and rep['coherent_ms'] > 0
