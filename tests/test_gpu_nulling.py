"""Null steering on the GPU (gpsmi_nul_*, csrc/gpsmi_nul.hip) against the float64 restatement
(tests/nul_ref.py), and what it buys: acquisition and tracking through a wideband jammer 30 dB over
the noise that leaves a single antenna nothing to find."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import nul_ref as R
from nul_ref import A4, array_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, JN_DB = 0.015, 20.0      # the matrix: noise of 1.9 LSB, every jammer 20 dB over it (7 of them: no clipping)
NS = (2048, 4096 + 32, 130944)
# what the float64 reference followed by the oracle's sweep finds on the jammed scene (determined on
# the CPU: nul_ref.NullRef, then gps_oracle.sweep_all_sats at the receiver's IT_SWEEP_ALL = 10 bins per
# block, 5 blocks): PRN -> (bin, code phase); CLEAN: the same sweep on the single-antenna scene without
# the jammer.  PRN 4 stands 3 degrees from the jammer and goes with it.
NULLED = {6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963), 24: (-3000.0, 150),
          27: (-3600.0, 1305), 28: (-2000.0, 1877), 32: (-2200.0, 1714)}
CLEAN = {4: (-2000.0, 143), 6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963),
         24: (-2800.0, 150), 27: (-3800.0, 1305), 28: (-2000.0, 1876), 32: (-2200.0, 1714)}
_CACHE = {}


def _cfg(n):
    from gpsmi.engine import Config
    for cs, n_cyc in ((2048, n // 2048), (16368, n // 16368), (n, 1)):
        if n_cyc >= 1 and cs * n_cyc == n:
            return Config(code_samples=cs, n_cyc=n_cyc)
    raise ValueError(n)


def _case_blocks(A, n, nb, raw_u8, mix=None):
    """[A][nb * n] of the matrix: by block length and blocks per call the jammer counts 0, 1 and A - 1,
    an all-zero block among noisy ones (raw input cannot hold a zero: the recorder's mid level on every
    antenna instead, copies as well) and a block whose antennas are exact copies of one another.
    mix: which of the three mixes (default: the one of the matrix's block length n)."""
    rng = np.random.default_rng(1000 * A + n % 997 + 7 * nb + raw_u8)
    k = NS.index(n) if mix is None else mix
    counts = (0, 1, A - 1)

    def noisy(j):
        return R.noisy_block(rng, A, n, j, JN_DB, SIGMA)

    def copies():
        return np.tile(SIGMA * 10.0 * R.cgauss(rng, n), (A, 1))

    def silent():
        return np.zeros((A, n), dtype=np.complex128)

    if nb == 1:
        blocks = [noisy(counts[k])]
    else:
        blocks = [[noisy(1), silent(), noisy(A - 1)], [noisy(0), copies(), noisy(1)],
                  [noisy(A - 1), silent(), copies()]][k]
    x = np.concatenate(blocks, axis=1)
    return R.quantise(x) if raw_u8 else x.astype(np.complex64)


CASES = [(A, n, raw_u8, nb) for A in (2, 3, 5, 8) for n in NS for raw_u8 in (False, True) for nb in (1, 3)]


@pytest.mark.parametrize('A,n,raw_u8,nb', CASES,
                         ids=[f'A{A}-n{n}-{"u8" if u else "c64"}-nb{nb}' for A, n, u, nb in CASES])
def test_case_matrix_against_the_reference(A, n, raw_u8, nb):
    """Flags exact; gain_db, weights and output within four times what a plain numpy evaluation of the
    header's formulas (nul_ref.plain) deviates from the restatement on the same case."""
    from gpsmi.nulling import NullSteer
    x = _case_blocks(A, n, nb, raw_u8)
    ns = NullSteer(_cfg(n), antennas=A, raw_u8=raw_u8)
    y = ns.apply(x).reshape(nb, n)
    flags, gain, w = ns.last_flags.copy(), ns.last_gain_db.copy(), ns.last_weights.copy()
    ns.close()
    y_r, f_r, g_r, w_r = R.NullRef(n, A).run(x)
    xc = (R.decode(x) if raw_u8 else x).reshape(A, nb, n)
    pl = [R.plain(xc[:, b], n) for b in range(nb)]
    assert [p[1] for p in pl] == f_r.tolist()
    assert (np.abs(g_r.astype(np.float64) - 3.0) >= 1.0).all(), g_r      # (no case near the threshold)
    tol_y = 4.0 * max(np.abs(p[0] - y_r[b]).max() for b, p in enumerate(pl))
    tol_g = 4.0 * max(abs(float(p[2]) - float(g_r[b])) for b, p in enumerate(pl))
    tol_w = 4.0 * max(np.abs(p[3] - w_r[b]).max() for b, p in enumerate(pl))
    dev_y = np.abs(y - y_r).max()
    dev_g = np.abs(gain.astype(np.float64) - g_r).max()
    dev_w = np.abs(w - w_r).max()
    print(f'nul-matrix A={A} n={n} {"u8" if raw_u8 else "c64"} nb={nb} flags={f_r.tolist()} '
          f'gain_db={np.round(g_r, 2).tolist()} dev_w={dev_w:.3g} tol_w={tol_w:.3g} dev_g={dev_g:.3g} '
          f'tol_g={tol_g:.3g} dev_y={dev_y:.3g} tol_y={tol_y:.3g}')
    assert np.array_equal(flags, f_r), (flags, f_r)
    assert dev_g <= tol_g and dev_w <= tol_w and dev_y <= tol_y
    for b in range(nb):
        if not f_r[b]:                                   # pass-through: antenna 0 bit for bit, e0
            assert y[b].tobytes() == xc[0, b].tobytes() and np.array_equal(w[b], np.eye(A)[0])


def _four_blocks(A=3, n=4096 + 32, raw_u8=False):
    rng = np.random.default_rng(11)
    x = np.concatenate([R.noisy_block(rng, A, n, j, JN_DB, SIGMA) for j in (1, 0, 2, 1)], axis=1)
    return R.quantise(x) if raw_u8 else x.astype(np.complex64)


def _results(ns):
    return ns.last_flags.tobytes() + ns.last_gain_db.tobytes() + ns.last_weights.tobytes()


def test_cut_of_the_call_format_entry_point_and_handle_do_not_change_the_bits():
    from gpsmi._lib import EngineError
    from gpsmi.engine import DeviceBuffer
    from gpsmi.nulling import NullSteer
    A, n = 3, 4096 + 32
    cfg = _cfg(n)
    raw = _four_blocks(A, n, True)
    x = R.decode(raw)
    a, b, u = NullSteer(cfg, antennas=A), NullSteer(cfg, antennas=A), NullSteer(cfg, antennas=A, raw_u8=True)
    y4 = a.apply(x)
    res4 = _results(a)
    assert a.last_flags.tolist() == [1, 0, 1, 1]
    # a pass-through block is antenna 0's decode
    assert y4[1].tobytes() == x[0, n:2 * n].tobytes()
    # one call of 4 blocks equals 4 calls of 1
    singles, res1 = [], []
    for k in range(4):
        singles.append(a.apply(np.ascontiguousarray(x[:, k * n:(k + 1) * n])))
        res1.append((a.last_flags.copy(), a.last_gain_db.copy(), a.last_weights.copy()))
    assert np.stack(singles).tobytes() == y4.tobytes()
    assert b''.join(r[i].tobytes() for i in range(3) for r in res1) == res4
    # two handles in one process agree
    assert b.apply(x).tobytes() == y4.tobytes() and _results(b) == res4
    # raw u8 equals complex64 of its decode
    assert u.apply(raw).tobytes() == y4.tobytes() and _results(u) == res4
    # apply equals apply_dev, in both formats
    for h, src in ((b, x), (u, raw)):
        d_in, d_out = DeviceBuffer(src.nbytes), DeviceBuffer(4 * n * 8)
        d_in.upload(src)
        h.apply_dev(d_in.ptr, d_out.ptr, 4)
        assert d_out.download(np.complex64, 4 * n).tobytes() == y4.tobytes() and _results(h) == res4
        # refusals on a live handle leave it usable
        with pytest.raises(EngineError, match='overlap'):
            h.apply_dev(d_in.ptr, d_in.ptr, 1)
        with pytest.raises(EngineError, match='overlap'):
            h.apply_dev(d_in.ptr, d_in.at(A * n * src.itemsize - 16), 1)   # (the tail of a call of 1)
        for nb in (0, -1):
            with pytest.raises(EngineError, match='nb out of range'):
                h._call('apply_dev', h.h, d_in.ptr, d_out.ptr, nb, None, None, None)
        with pytest.raises(EngineError, match='aligned'):
            h.apply_dev(d_in.ptr, d_out.at(8), 1)
        with pytest.raises(EngineError, match='aligned'):
            h.apply_dev(d_in.at(2), d_out.ptr, 1)
        h.apply_dev(d_in.ptr, d_out.ptr, 4)
        assert d_out.download(np.complex64, 4 * n).tobytes() == y4.tobytes() and _results(h) == res4
        assert h.last_ms() > 0
        d_in.free()
        d_out.free()
    for h in (a, b, u):
        h.close()


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_handle_reuse_and_create_destroy_cycles(raw_u8):
    """1, 3, 1 blocks on one handle equal each call on a fresh one (the buffers grow and are kept), a
    refused call in between changes nothing, and handles come and go."""
    from gpsmi._lib import EngineError
    from gpsmi.nulling import NullSteer
    A, n = 5, 2048
    cfg = _cfg(n)
    rng = np.random.default_rng(21)
    z = np.concatenate([R.noisy_block(rng, A, n, j, JN_DB, SIGMA) for j in (2, 0, 4)], axis=1)
    x = R.quantise(z) if raw_u8 else z.astype(np.complex64)

    def make():
        return NullSteer(cfg, antennas=A, raw_u8=raw_u8)

    def run(h, nb):
        out = h.apply(np.ascontiguousarray(x.reshape(A, 3, n)[:, :nb]))
        return out.tobytes() + _results(h)

    reused = make()
    for nb in (1, 3, 1):
        fresh = make()
        want = run(fresh, nb)
        fresh.close()
        with pytest.raises(EngineError):
            reused._call('apply', reused.h, None, None, nb, None, None, None)
        assert run(reused, nb) == want
    reused.close()
    for _ in range(8):
        h = make()
        h.close()
        h.close()                                        # (closing twice is harmless)


def _jammed(b, raw_u8=False):
    """Block b of the jammed scene, [4][NGPS]: rendered once, as the recorder would write it."""
    from gpsmi import synth
    if ('raw', b) not in _CACHE:
        _CACHE['raw', b] = array_scene().block_raw(b)
        _CACHE['c64', b] = synth.raw_to_c64(_CACHE['raw', b])
    return _CACHE['raw' if raw_u8 else 'c64', b]


def _sweep(acq, blocks, cfg, prns):
    freq, lst, found, ready, i = cfg.min_freq, list(prns), [], False, 0
    while not ready:
        ready, freq, found = acq.sweepAllSats(blocks(i), freq, lst, found, itSweep=cfg.it_sweep_all)
        i += 1
    return {s: (f, d) for _, s, f, d in found}


def test_acquisition_through_the_wideband_jammer():
    """Antenna 0 alone finds none of the eight satellites; behind the null steering the sweep finds
    exactly what the float64 reference followed by the oracle's search finds, at the clean scene's
    bins (or the neighbour, for a satellite between two bins) and code phases +-1."""
    from gpsmi.acquisition import Acquisition
    from gpsmi.engine import Config
    from gpsmi.nulling import NullSteer
    cfg = Config()
    arr = array_scene()
    prns = [s.prn for s in arr.scene.sats] + [1]
    acq = Acquisition(cfg)
    assert _sweep(acq, lambda i: np.ascontiguousarray(_jammed(i)[0]), cfg, prns) == {}
    ns = NullSteer(cfg, antennas=A4)
    found = _sweep(acq, lambda i: ns.apply(_jammed(i)), cfg, prns)
    assert ns.last_flags[0] == 1 and 27.0 < ns.last_gain_db[0] < 28.5
    ns.close()
    acq.engine.close()
    assert set(found) == set(NULLED) and len(found) >= 6
    for s, (f, d) in found.items():
        assert abs(f - CLEAN[s][0]) <= cfg.step_freq, (s, f, d)
        dd = abs(d - CLEAN[s][1])
        assert min(dd, cfg.code_samples - dd) <= 1, (s, f, d)
        dd = abs(d - NULLED[s][1])
        assert abs(f - NULLED[s][0]) <= cfg.step_freq and min(dd, cfg.code_samples - dd) <= 1, (s, f, d)


N_BLOCKS = 94                   # 3 s of signal


def test_receiver_with_null_steering_locks_what_the_reference_finds():
    from gpsmi.pipeline import Receiver
    rx = Receiver(antennas=A4, null=True)
    for b in range(N_BLOCKS):
        rx.feed(_jammed(b))
    rx.drain()
    assert set(rx.act_sat_set) == set(NULLED)
    locked = [rx.pool.trk.get_state(w)['phase_locked'] != 0 for w, s in enumerate(rx.pool_worker) if s]
    assert len(locked) == len(NULLED) and all(locked)
    assert len(rx.result_list) >= 1
    assert {f['SAT'] for f in pickle.loads(rx.result_list[-1])[1]} == set(NULLED)
    assert rx.nuller.last_flags[0] == 1
    rx.close()


def test_receiver_without_the_option_is_unchanged():
    """Receiver() with the new keywords at their defaults returns what Receiver on the same blocks
    returns without them, byte for byte, and makes no stage."""
    from gpsmi.pipeline import Receiver
    sc = array_scene(False).scene
    rx_a, rx_b = Receiver(antennas=1, null=None), Receiver()
    assert rx_a.nuller is None and not rx_a.conditioner and not rx_b.conditioner
    for b in range(40):
        x = sc.block(b)
        assert rx_a.feed(x) == rx_b.feed(x)
    rx_a.drain()
    rx_b.drain()
    assert rx_a.result_list == rx_b.result_list and len(rx_a.result_list) >= 1
    assert set(rx_a.act_sat_set) == {s.prn for s in sc.sats}
    rx_a.close()
    rx_b.close()


def test_run_file_null_on_four_raw_recordings(tmp_path):
    """tools/run_file.py --antenna ... --null on the jammed scene written as four raw files: the flag
    and the gain of every block, and the satellites of the reference acquired and tracked.  (Three
    seconds hold no complete subframe 1-3: the position fix of a --null run is the solver's work on
    the same datagrams as without it, tests/test_run_file.py.)"""
    paths = [str(tmp_path / f'ant{a}.bin') for a in range(A4)]
    files = [open(p, 'wb') for p in paths]
    for b in range(N_BLOCKS):
        raw = _jammed(b, raw_u8=True)
        for a, f in enumerate(files):
            raw[a].astype('<u2').tofile(f)
    for f in files:
        f.close()
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), paths[0], '--null', '--json']
    for p in paths[1:]:
        cmd += ['--antenna', p]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['blocks'] == N_BLOCKS and out['datagrams'] >= 1
    assert out['null']['antennas'] == A4 and out['null']['flags'] == [1] * N_BLOCKS
    assert all(27.0 < g < 28.5 for g in out['null']['gain_db'])
    assert {s for s, _, _ in out['acquired']} == set(NULLED)
    assert sorted(out['tracked']) == sorted(NULLED)
