"""GPU: the deep search that keeps its surfaces (gpsmi_acq_search_deep_rows_dev), the collective
kernels against the numpy restatement (collective_ref.py) byte for byte, and snapshot_fix with
collective=True on the weak scene of test_collective.py (eight satellites at 24 dB-Hz, a-priori
10 km and 1 s off).

Rows against records.  argmax and peak are recomputed from a row exactly.  mean and std are not a
function of the rounded row alone (at 2048 the record's mean adds unrounded products, the pinned
sum of gpsmi_acq_search.h; at 16368 the variance is E[m^2] - mean^2 of float32 partial sums), so
they are held to the rounding of their own sums against float64 on the row: at most 24 float32
roundings lie between a record's mean and the exact one (15 additions at 2048, 22 at 16368, the
scale, the magnitudes' own rounding): 24 * 2^-24 relative.  A std carries the same roundings in
every squared term and, at 16368, the cancellation of mean^2: 64 * 2^-24 * (1 + (mean / std)^2).

End to end.  The restatement's fix on the scene is 14.67 m from the truth (test_collective.py); the
GPU's may be twice that, for the float32 differences between the restated search and the kernels
that test_gpu_acq_deep.py tolerates."""
import ctypes as C

import numpy as np
import pytest

import collective_ref as R
from test_collective import SCENE_CN0, SCENE_FIX_ERROR_M
from test_gpu_acq_noncoherent import CFG, _engine, _same, _upload

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ---- 1. the rows call ----------------------------------------------------------------------------

def _rows_call(e, data, prns, freqs, n_coh, n_seg, f_offset):
    from gpsmi.engine import DeviceBuffer
    cs = e.cfg.code_samples
    rows = DeviceBuffer(len(prns) * len(freqs) * cs * 4)
    try:
        tab = e.search_deep(data, prns, freqs, n_coh, n_seg, f_offset=f_offset, rows=rows)
        return tab, rows.download(np.float32, len(prns) * len(freqs) * cs).reshape(len(prns), len(freqs), cs)
    finally:
        rows.free()


@pytest.mark.parametrize('cs, prns, freqs, n_coh, n_seg', [
    (2048, [6, 15, 3], [-4800.0, -4200.0, 0.0, 4200.0, 4800.0], 4, 25),
    (16368, [6, 29], [-4800.0, 0.0, 4200.0], 2, 4)])
def test_rows_are_what_the_records_are_statistics_of(cs, prns, freqs, n_coh, n_seg):
    from deep_ref import deep_scene, deep_shifts
    from gpsmi.synth import raw_to_c64
    f_offset = 250e3                                   # shifts of several samples per segment
    assert np.all(deep_shifts(freqs, n_coh, n_seg, cs, f_offset=f_offset)[:, 1:] % cs != 0)
    n = n_seg * n_coh * cs
    raw = deep_scene(cs, CFG[cs]['n_cyc'], amp=0.05).block_raw(0, n=n)
    c64 = raw_to_c64(raw)
    e, er = _engine(cs), _engine(cs, raw_u8=True)
    try:
        ref = e.search_deep(c64, prns, freqs, n_coh, n_seg, f_offset=f_offset)
        tab, rows = _rows_call(e, c64, prns, freqs, n_coh, n_seg, f_offset)
        assert e.last_ms() > 0
        _same(tab, ref)                                # the records: search_deep's, byte for byte
        tab_r, rows_r = _rows_call(er, raw, prns, freqs, n_coh, n_seg, f_offset)
        _same(tab_r, ref)
        _same(rows_r, rows)                            # raw u8 input: the same bytes
        buf = _upload(c64)                             # device-resident input
        try:
            tab_d, rows_d = _rows_call(e, (buf.ptr, n), prns, freqs, n_coh, n_seg, f_offset)
        finally:
            buf.free()
        _same(tab_d, ref)
        _same(rows_d, rows)
        _same(e.search_deep(c64, prns, freqs, n_coh, n_seg, f_offset=f_offset), ref)      # (and nothing lingers)
    finally:
        e.close()
        er.close()
    assert np.isfinite(rows).all() and (rows >= 0).all()
    worst = [0.0, 0.0]
    for j in range(len(prns)):
        for b in range(len(freqs)):
            row, rec = rows[j, b], ref[b, j]
            assert rec['argmax'] == int(np.argmax(row)) and rec['peak'] == row[rec['argmax']]
            mean, std = row.astype(np.float64).mean(), row.astype(np.float64).std()
            dm, ds = abs(rec['mean'] - mean) / mean, abs(rec['std'] - std) / std
            worst = [max(worst[0], dm / (24 * EPS)), max(worst[1], ds / (64 * EPS * (1 + (mean / std) ** 2)))]
            assert dm <= 24 * EPS and ds <= 64 * EPS * (1 + (mean / std) ** 2)
    print('cs %d: mean within %.2f of its bound, std within %.3f of its bound' % (cs, *worst))


def test_rows_argument_errors():
    from deep_ref import deep_scene
    from gpsmi.engine import DeviceBuffer, EngineError
    from gpsmi._lib import PEAK_DTYPE, ptr
    e, e16 = _engine(2048), _engine(16368)
    data = deep_scene(amp=0.05).block(0, n=2 * 2 * 2048)
    buf, small = _upload(data), DeviceBuffer(16)
    try:
        prn, f = np.array([3, 6], np.int32), np.array([0.0, 200.0])
        out = np.zeros((2, 2), PEAK_DTYPE)
        rc = e.lib.gpsmi_acq_search_deep_rows_dev(e.h, buf.ptr, data.size, ptr(prn), 2, ptr(f), 2, 2, 2, 1575.42e6, 0.0,
                                                  ptr(out), None, None)
        assert rc == -1 and b'd_rows' in e.lib.gpsmi_last_error()
        with pytest.raises(ValueError):                # a buffer too small never reaches the kernel
            e.search_deep(data, [3, 6], [0.0, 200.0], 2, 2, rows=small)
        with pytest.raises(ValueError):
            e.search_deep(data, [3, 6], [0.0, 200.0], 2, 2, rows=small, nbr=True)
        # one segment at 16368 is the coherent search: no surface
        d16 = deep_scene(16368, 8, amp=0.05).block(0, n=2 * 16368)
        rows = DeviceBuffer(16368 * 4)
        try:
            with pytest.raises(EngineError, match=r'\(-5\)'):
                e16.search_deep(d16, [3], [0.0], 2, 1, rows=rows)
        finally:
            rows.free()
    finally:
        buf.free()
        small.free()
        e.close()
        e16.close()


# ---- 2. the collective kernels against the restatement, byte for byte ---------------------------------

NORMAL, STEEP = 'normal', 'steep'
CASES = [
    # cs, nsat, (n_e, n_n, n_t), pool, gradients
    (2048, 1, (1, 1, 1), 1, NORMAL),
    (2048, 5, (67, 33, 1), 1, NORMAL),                 # windows in LDS, four rounds of lags per chunk
    (2048, 5, (67, 33, 1), 3, NORMAL),                 # 3 does not divide 2048
    (2048, 32, (3, 5, 2), 1, NORMAL),
    (2048, 32, (67, 33, 1), 8, NORMAL),                # 32 windows of 505 lags do not fit: through L2
    (2048, 5, (3, 5, 2), 8, STEEP),                    # x_p negative and beyond 2 cs: through L2
    (2048, 5, (3, 5, 2), 1, STEEP),
    (16368, 1, (1, 1, 1), 3, NORMAL),
    (16368, 5, (67, 33, 1), 8, NORMAL),
    (16368, 32, (3, 5, 2), 1, NORMAL),
    (16368, 5, (3, 5, 2), 1, STEEP),
]


@pytest.fixture(scope='module')
def random_rows():
    """Random float32 surfaces [32][3][cs] per code length, made once: positive, a row with equal
    maxima, a flat bin inside a window, and a satellite all of whose bins are flat."""
    out = {}
    for cs in (2048, 16368):
        rng = np.random.default_rng(cs)
        rows = (1.0 + 0.2 * rng.random((32, 3, cs), dtype=np.float32)).astype(np.float32)
        rows[0, 0, [5, cs // 2, cs - 1]] = 2.0                                # equal maxima
        rows[1, 1] = 0.75                                                     # std 0 inside a window
        rows[2] = 1.5                                                         # nothing but flat bins
        out[cs] = rows
    return out


def _case_args(cs, nsat, shape, pool, kind):
    rng = np.random.default_rng(1000 * nsat + pool + cs)
    sats = np.zeros(nsat, R.SAT_DTYPE)
    sats['row'] = rng.permutation(32)[:nsat] if nsat > 1 else 0               # (row 0: the equal maxima)
    if nsat >= 5:
        sats['row'][:3] = [0, 1, 2]
    lo = rng.integers(0, 3, nsat)
    sats['bin_lo'], sats['bin_hi'] = lo, np.maximum(lo, rng.integers(0, 3, nsat))
    sats['bin_lo'][0] = sats['bin_hi'][0] = 0                                 # one bin
    if nsat >= 5:
        sats['bin_lo'][1:3], sats['bin_hi'][1:3] = 0, 2                       # the full window
    sats['lag0'] = rng.uniform(-3.0 * cs, 3.0 * cs, nsat)
    if nsat >= 5:
        sats['lag0'][3:5] = [-2.5 * cs - 0.5, 2.5 * cs + 0.5]                 # below 0, beyond 2 cs, on a half
    k = 1.0 if kind == NORMAL else 2000.0
    sats['g_e'], sats['g_n'] = k * rng.uniform(-0.0068, 0.0068, (2, nsat))
    sats['g_t'] = k * rng.uniform(-5.5, 5.5, nsat)
    n_e, n_n, n_t = shape
    grid = dict(n_e=n_e, n_n=n_n, n_t=n_t, pool=pool, e0=-0.5 * n_e * 293.0 + 11.0, n0=-0.5 * n_n * 293.0 - 7.0,
                t0=-0.4, d_e=293.0, d_n=293.0, d_t=0.8)
    return sats, grid


@pytest.mark.parametrize('cs, nsat, shape, pool, kind', CASES)
def test_cell_map_equals_the_restatement(random_rows, cs, nsat, shape, pool, kind):
    rows = random_rows[cs]
    sats, grid = _case_args(cs, nsat, shape, pool, kind)
    if kind == STEEP:                                                         # the case is what it says
        E = grid['e0'] + np.arange(grid['n_e']) * grid['d_e']
        x = sats['lag0'][:, None] + sats['g_e'][:, None] * E[None, :]
        assert x.min() < 0 and x.max() > 2 * cs
    ref = R.collective(rows, sats, grid)
    e = _engine(cs)
    buf = _upload(rows)
    try:
        got = e.collective(buf, sats, grid, nsv_rows=32, nbins=3)
        assert e.last_ms() > 0
        again = e.collective(buf, sats, grid, nsv_rows=32, nbins=3)
    finally:
        buf.free()
        e.close()
    assert got.shape == ref.shape == shape[::-1] and got.dtype == ref.dtype
    assert np.isfinite(got['score']).all()
    bad = np.flatnonzero(got.ravel() != ref.ravel())
    assert bad.size == 0, (bad[:5], got.ravel()[bad[:5]], ref.ravel()[bad[:5]])
    _same(got, ref)
    _same(again, got)


def test_collective_argument_errors(random_rows):
    from gpsmi.engine import EngineError
    rows = random_rows[2048]
    sats, grid = _case_args(2048, 5, (3, 5, 2), 1, NORMAL)
    e = _engine(2048)
    buf = _upload(rows)
    try:
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.collective(buf, sats, dict(grid, pool=0), nsv_rows=32, nbins=3)
        with pytest.raises(EngineError, match=r'\(-1\)'):
            e.collective(buf, sats, grid, nsv_rows=32, nbins=2)               # a window past the bins
        with pytest.raises(EngineError, match=r'\(-5\)'):
            e.collective(buf, sats, dict(grid, n_e=4096, n_n=2048), nsv_rows=32, nbins=3)
        with pytest.raises(ValueError):
            e.collective(buf, sats, grid, nsv_rows=33, nbins=3)               # more rows than the buffer holds
        _same(e.collective(buf, sats, grid, nsv_rows=32, nbins=3), R.collective(rows, sats, grid))
    finally:
        buf.free()
        e.close()


# ---- 3. end to end on the weak scene -------------------------------------------------------------------

@pytest.fixture(scope='module')
def weak():
    """The scene at SCENE_CN0 and the restatement's search on it, once."""
    from gpsmi.engine import Config
    sc, info, data = R.weak_scene(SCENE_CN0)
    prns, freqs, bins, rows = R.scene_search(data, info, Config())
    pos, t = R.scene_apriori(info)
    res = R.pyramid(rows, info['ephs'], prns, bins, t, pos, R.SCENE_RADIUS_M, R.SCENE_TIME_S)
    return sc, info, data, pos, t, prns, freqs, bins, rows, res


def test_weak_scene_needs_the_collective_search(weak):
    from gpsmi import snapshot as S
    from gpsmi.acquisition import Acquisition
    sc, info, data, pos, t, prns, freqs, bins, rows, res = weak
    ref_meas, _ = S.collective_records(lambda p: rows[bins[p][0], bins[p][1]:bins[p][2] + 1], prns,
                                       [freqs[b[1]:b[2] + 1] for b in bins], res['model'], res['lag'], 2048)
    acq = Acquisition()
    try:
        plain, meas0, _ = S.snapshot_fix(acq, data, info['ephs'], t, pos=pos)
        print('without the option: %d satellites measured, %s' % (len(meas0), plain.reason))
        assert not plain.ok and plain.ecef is None and plain.path == 'measure' and len(meas0) < S.MIN_SAT
        stats = {}
        fix, meas, ms = S.snapshot_fix(acq, data, info['ephs'], t, pos=pos, collective=True, stats=stats,
                                       collective_cfg=dict(radius_m=R.SCENE_RADIUS_M, time_s=R.SCENE_TIME_S))
    finally:
        acq.engine.close()
    got = stats['collective']
    err = np.linalg.norm(fix.ecef - info['truth']) if fix.ok else float('nan')
    print('collective: levels %s, margin %.1f, %d measured, fix %s %.2f m from the truth (restatement %.2f m), '
          'device ms per level %s' % ([l['best'] for l in got['levels']], got['margin'], len(meas),
                                      fix.ok or fix.reason, err, SCENE_FIX_ERROR_M, np.round(got['level_ms'], 3)))
    assert got['prns'] == prns
    assert [l['best'] for l in got['levels']] == [l['best'] for l in res['levels']]          # the same best cells
    assert np.linalg.norm(got['ecef'] - res['ecef']) < 1e-6 and abs(got['t_gps'] - res['t_gps']) < 1e-9
    assert meas['prn'].tolist() == ref_meas['prn'].tolist()                                  # the same satellites
    assert fix.ok and fix.path == 'collective' and sorted(fix.prns) == ref_meas['prn'].tolist()
    assert err <= 2.0 * SCENE_FIX_ERROR_M
    assert ms > 0 and len(got['level_ms']) == 4 and min(got['level_ms']) > 0


# ---- 4. without the option nothing changes ----------------------------------------------------------------

def test_without_the_option_every_byte_is_as_before():
    """snapshot_fix on test_gpu_snapshot.py's strong scene: the default call, collective=None and
    collective=False, and the chain as it was before the option existed (measure -> doppler_fix ->
    coarse_time_fix, composed here) give the same measurements and the same fix, byte for byte."""
    import snapshot_truth as T
    from gpsmi import snapshot as S
    from gpsmi.acquisition import Acquisition
    _, info = T.strong()
    raw = T.raw('strong')
    t = info['t0_gps'] + 20.0
    acq = Acquisition(raw_u8=True)
    try:
        base = S.snapshot_fix(acq, raw, info['ephs'], t)
        forms = [S.snapshot_fix(acq, raw, info['ephs'], t, collective=None),
                 S.snapshot_fix(acq, raw, info['ephs'], t, collective=False)]
        meas = S.measure(acq, raw, prns=sorted(info['ephs']))
        pos, _ = S.doppler_fix(meas, info['ephs'], t)
        ref = int(np.argmax(S.cn0_weights(meas['cn0_dbhz'])))
        before = S.coarse_time_fix(meas, info['ephs'], float(t) + int(meas['sample'][ref]) / 2048000.0, pos)
        # with an a-priori and enough satellites the option does not run either
        with_pos = S.snapshot_fix(acq, raw, info['ephs'], t, pos=T.TRUTH + 1.0e3)
        opt = S.snapshot_fix(acq, raw, info['ephs'], t, pos=T.TRUTH + 1.0e3, collective=True)
    finally:
        acq.engine.close()

    def same_fix(a, b):
        assert a.ok and b.ok and a.path == b.path == 'measure'
        assert a.ecef.tobytes() == b.ecef.tobytes() and a.residuals.tobytes() == b.residuals.tobytes()
        assert (a.t_gps, a.sample, a.prns, a.ref_prn, a.dropped, a.g, a.rms_m, a.bias_m) == \
               (b.t_gps, b.sample, b.prns, b.ref_prn, b.dropped, b.g, b.rms_m, b.bias_m)
    assert len(base[1]) == 8
    for fx, m, _ in forms:
        assert m.tobytes() == base[1].tobytes()
        same_fix(fx, base[0])
    assert meas.tobytes() == base[1].tobytes()
    same_fix(before, base[0])
    assert opt[1].tobytes() == with_pos[1].tobytes()
    same_fix(opt[0], with_pos[0])


# ---- 5. tools/run_file.py --collective -------------------------------------------------------------------

def test_run_file_collective(weak, tmp_path):
    """The weak scene as a recording: --snapshot with --collective gets the fix snapshot_fix gets, and
    says which path made it; the flag without --snapshot or --near is refused."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from gpsmi import position as P
    sc, info, data, pos, t = weak[:5]
    path = str(tmp_path / 'weak.bin')
    n = len(data)
    with open(path, 'wb') as f:                       # 32 whole blocks: the second and 48 ms more
        sc.block_raw(0, n=n).astype('<u2').tofile(f)
        sc.block_raw(31)[n - 31 * 65536:].astype('<u2').tofile(f)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    tool = [sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path]
    near = ','.join(repr(float(v)) for v in P.ecef_to_geo(pos))
    r = subprocess.run(tool + ['--snapshot', '1.0', '--ephemeris', eph, '--time', repr(t), '--near', near,
                               '--collective', '15', '--json'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])['snapshot']
    err = float(np.linalg.norm(np.array(s['position']['ecef_m']) - info['truth'])) if s['ok'] else float('nan')
    print('run_file --collective: ok %s %s, path %s, %.2f m from the truth, %s' % (s['ok'], s['reason'], s['path'], err,
                                                                                 s['collective']))
    assert s['ok'] and s['path'] == 'collective' and s['satellites'] == weak[5]
    assert err <= 2.0 * SCENE_FIX_ERROR_M and len(s['collective']['level_ms']) == 4
    for bad in (['--collective'], ['--snapshot', '1.0', '--ephemeris', eph, '--time', repr(t), '--collective']):
        r = subprocess.run(tool + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and '--collective' in r.stderr
