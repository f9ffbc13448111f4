"""Space-time null steering on the GPU (gpsmi_nul_cfg.taps, csrc/gpsmi_nul_stap.h) against its
restatement (tests/stap_ref.py), and what it buys: acquisition and tracking through a wideband jammer
that reaches the two antennas through channels 0.3 samples apart in delay."""
import numpy as np
import pytest

import nul_ref as R
import stap_ref as S

pytestmark = pytest.mark.gpu

SIGMA, JN_DB = 0.015, 20.0      # as tests/test_gpu_nulling.py: noise of 1.9 LSB, every jammer 20 dB over it
NS = (2048, 4096 + 32, 130944)  # one slice of the covariance, one slice that ends inside a staged chunk, 16 slices
LONG = ((2, 3), (5, 5), (8, 7))


def _cfg(n):
    from gpsmi.engine import Config
    for cs, n_cyc in ((2048, n // 2048), (16368, n // 16368), (n, 1)):
        if n_cyc >= 1 and cs * n_cyc == n:
            return Config(code_samples=cs, n_cyc=n_cyc)
    raise ValueError(n)


def _case_blocks(A, T, n, nb, raw_u8):
    """[A][nb * n] of the matrix, after test_gpu_nulling._case_blocks: by block length and blocks per
    call the jammer counts 0, 1 and A - 1, an all-zero block among noisy ones (raw input: the recorder's
    mid level on every antenna, copies as well) and a block whose antennas are exact copies of one
    another.  The jammers are stap_ref.jammer's: tones, and white noise through a two-tap filter of its
    own per antenna; which kind comes first alternates with the case."""
    rng = np.random.default_rng(100000 * T + 1000 * A + n % 997 + 7 * nb + raw_u8)
    k = NS.index(n)
    counts = (0, 1, A - 1)
    first = ('filtered', 'tone')[(A + T + k + nb) % 2]

    def noisy(j):
        return S.stap_block(rng, A, n, j, JN_DB, SIGMA, first)

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


CASES = [(A, T, n, raw_u8, nb) for A in (2, 3, 5, 8) for T in (3, 5, 7) for n in NS
         for raw_u8 in (False, True) for nb in (1, 3) if n != NS[2] or (A, T) in LONG]


def case_reference(A, T, n, raw_u8, nb):
    """(x, decoded x [A][nb][n], extended-precision restatement, ascending float64 restatement, plain)
    of one case; each of the last three is (y [nb][n], flags, gain_db, w [nb][A][T])."""
    x = _case_blocks(A, T, n, nb, raw_u8)
    xc = (R.decode(x) if raw_u8 else x).reshape(A, nb, n)
    ref = S.StapRef(n, A, T)
    ext, asc = ref.run(x, 'ext'), ref.run(x, 'f64')
    pl = [S.plain(xc[:, b], n, T) for b in range(nb)]
    pl = (np.stack([p[0] for p in pl]), np.array([p[1] for p in pl], dtype=np.int32),
          np.array([p[2] for p in pl], dtype=np.float32), np.stack([p[3] for p in pl]))
    return x, xc, ext, asc, pl


def case_bounds(ext, asc, pl):
    """(tol_w, tol_g, tol_y): four times the larger deviation of the two other evaluations from the
    extended-precision one; gain_db floored at one float32 unit in the last place."""
    tol = [4.0 * max(np.abs(o[i].astype(np.complex128) - ext[i]).max() for o in (asc, pl)) for i in (3, 2, 0)]
    tol[1] = max(tol[1], float(np.spacing(np.abs(ext[2]).astype(np.float32)).max()))
    return tol


@pytest.mark.parametrize('A,T,n,raw_u8,nb', CASES,
                         ids=[f'A{A}-T{T}-n{n}-{"u8" if u else "c64"}-nb{nb}' for A, T, n, u, nb in CASES])
def test_case_matrix_against_the_restatement(A, T, n, raw_u8, nb):
    """Flags exact; the output byte for byte what combine() makes of the weights the GPU returned;
    weights, gain_db and output within four times what the ascending float64 sums and a plain numpy
    evaluation deviate from the extended-precision restatement on the same case."""
    from gpsmi.nulling import NullSteer
    x, xc, ext, asc, pl = case_reference(A, T, n, raw_u8, nb)
    y_e, f_e, g_e, w_e = ext
    ns = NullSteer(_cfg(n), antennas=A, raw_u8=raw_u8, taps=T)
    y = ns.apply(x).reshape(nb, n)
    flags, gain, w = ns.last_flags.copy(), ns.last_gain_db.copy(), ns.last_weights.copy()
    ns.close()
    assert f_e.tolist() == asc[1].tolist() == pl[1].tolist()
    assert (np.abs(g_e.astype(np.float64) - 3.0) >= 1.0).all(), g_e          # (no case near the threshold)
    tol_w, tol_g, tol_y = case_bounds(ext, asc, pl)
    assert tol_w <= 1e-6 * np.abs(w_e).max(), (tol_w, np.abs(w_e).max())     # (no mutation fits under it)
    assert w.shape == (nb, A, T)
    dev_w = np.abs(w - w_e).max()
    dev_g = np.abs(gain.astype(np.float64) - g_e).max()
    dev_y = np.abs(y - y_e).max()
    print(f'stap-matrix A={A} T={T} n={n} {"u8" if raw_u8 else "c64"} nb={nb} flags={f_e.tolist()} '
          f'gain_db={np.round(g_e, 2).tolist()} dev_w={dev_w:.3g} tol_w={tol_w:.3g} dev_g={dev_g:.3g} '
          f'tol_g={tol_g:.3g} dev_y={dev_y:.3g} tol_y={tol_y:.3g}')
    assert np.array_equal(flags, f_e), (flags, f_e)
    c = (T - 1) // 2
    for b in range(nb):
        if f_e[b]:
            assert y[b].tobytes() == S.combine(xc[:, b], w[b]).tobytes()
            assert not y[b, :c].any() and not y[b, n - c:].any() and w[b, 0, c] == 1.0
        else:                                            # pass-through: antenna 0 bit for bit, the unit vector
            e = np.zeros((A, T))
            e[0, c] = 1.0
            assert y[b].tobytes() == xc[0, b].tobytes() and np.array_equal(w[b], e)
    assert dev_g <= tol_g and dev_w <= tol_w and dev_y <= tol_y


def _four_blocks(A, n, raw_u8=False):
    rng = np.random.default_rng(11)
    x = np.concatenate([S.stap_block(rng, A, n, j, JN_DB, SIGMA, f)
                        for j, f in ((1, 'filtered'), (0, 'tone'), (2, 'tone'), (1, 'tone'))], axis=1)
    return R.quantise(x) if raw_u8 else x.astype(np.complex64)


def _results(ns):
    return ns.last_flags.tobytes() + ns.last_gain_db.tobytes() + ns.last_weights.tobytes()


def test_cut_of_the_call_format_entry_point_and_handle_do_not_change_the_bits():
    from gpsmi._lib import EngineError
    from gpsmi.engine import DeviceBuffer
    from gpsmi.nulling import NullSteer
    A, T, n = 3, 5, 3 * 8192 + 4096 + 32                  # (four slices, the last one short)
    cfg = _cfg(n)
    raw = _four_blocks(A, n, True)
    x = R.decode(raw)
    a, b = NullSteer(cfg, antennas=A, taps=T), NullSteer(cfg, antennas=A, taps=T)
    u = NullSteer(cfg, antennas=A, raw_u8=True, taps=T)
    y4 = a.apply(x)
    res4 = _results(a)
    assert a.last_flags.tolist() == [1, 0, 1, 1] and a.last_weights.shape == (4, A, T)
    assert y4[1].tobytes() == x[0, n:2 * n].tobytes()     # a pass-through block is antenna 0's decode
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
        with pytest.raises(EngineError, match='overlap'):  # refusals on a live handle leave it usable
            h.apply_dev(d_in.ptr, d_in.ptr, 1)
        with pytest.raises(EngineError, match='nb out of range'):
            h._call('apply_dev', h.h, d_in.ptr, d_out.ptr, 0, None, None, None)
        with pytest.raises(EngineError, match='aligned'):
            h.apply_dev(d_in.ptr, d_out.at(8), 1)
        h.apply_dev(d_in.ptr, d_out.ptr, 4)
        assert d_out.download(np.complex64, 4 * n).tobytes() == y4.tobytes() and _results(h) == res4
        assert h.last_ms() > 0
        d_in.free()
        d_out.free()
    for h in (a, b, u):
        h.close()


@pytest.mark.parametrize('raw_u8', [False, True], ids=['c64', 'u8'])
def test_handle_reuse_with_refused_calls_in_between(raw_u8):
    """1, 3, 1 blocks on one handle equal each call on a fresh one (the buffers grow and are kept), and
    a refused call in between changes nothing."""
    from gpsmi._lib import EngineError
    from gpsmi.nulling import NullSteer
    A, T, n = 5, 3, 2048
    cfg = _cfg(n)
    rng = np.random.default_rng(21)
    z = np.concatenate([S.stap_block(rng, A, n, j, JN_DB, SIGMA) for j in (2, 0, 4)], axis=1)
    x = R.quantise(z) if raw_u8 else z.astype(np.complex64)

    def make():
        return NullSteer(cfg, antennas=A, raw_u8=raw_u8, taps=T)

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
    assert reused.last_flags.tolist() == [1]
    reused.close()


def test_taps_0_and_1_are_the_one_weight_stage_byte_for_byte():
    """A taps = 1 handle and a taps = 0 handle give nul_ref.NullRef's bytes (output, flags, gain and
    weights) on a case of the existing stage's matrix: A = 3, n = 4128, complex64, three blocks."""
    import test_gpu_nulling as G
    from gpsmi.nulling import NullSteer
    A, n, nb = 3, 4096 + 32, 3
    x = G._case_blocks(A, n, nb, False)
    y_r, f_r, g_r, w_r = R.NullRef(n, A).run(x)
    assert f_r.tolist() == [0, 1, 1]
    for taps in (1, 0):
        ns = NullSteer(_cfg(n), antennas=A, taps=taps)
        y = ns.apply(x)
        assert ns.last_weights.shape == (nb, A)
        assert y.tobytes() == y_r.tobytes() and np.array_equal(ns.last_flags, f_r)
        assert ns.last_weights.tobytes() == w_r.tobytes() and ns.last_gain_db.tobytes() == g_r.tobytes()
        ns.close()


# ---- what the taps buy: scene (a) of tests/test_stap.py in raw u8 ---------------------------------

CLEAN = {4: (-2000.0, 143), 6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963),
         24: (-2800.0, 150), 27: (-3800.0, 1305), 28: (-2000.0, 1876), 32: (-2200.0, 1714)}
_RAW = {}


def _raw(b):
    """Block b of scene (a), uint16 [2][NGPS]: rendered once, as the recorder would write it."""
    if b not in _RAW:
        _RAW[b] = S.stap_scene('a').block_raw(b)
    return _RAW[b]


def _sweep(acq, blocks, cfg, prns):
    freq, lst, found, ready, i = cfg.min_freq, list(prns), [], False, 0
    while not ready:
        ready, freq, found = acq.sweepAllSats(blocks(i), freq, lst, found, itSweep=cfg.it_sweep_all)
        i += 1
    return {s: (f, d) for _, s, f, d in found}


def test_acquisition_through_a_jammer_behind_mismatched_channels():
    """Two antennas 0.3 samples apart in delay, a white jammer 30 dB over the noise: one weight per
    antenna leaves the sweep nothing (the CPU's empty set), five taps find what the restatement
    followed by the oracle's sweep finds, at the clean scene's bins (or the neighbour) and code
    phases +-1."""
    from gpsmi.acquisition import Acquisition
    from gpsmi.engine import Config
    from gpsmi.nulling import NullSteer
    cfg = Config()
    prns = [s.prn for s in S.stap_scene('a').scene.sats] + [1]
    acq = Acquisition(cfg)
    for taps, gain in ((1, (5.5, 7.5)), (5, (23.5, 26.0))):
        want = S.FOUND['a', True, taps]
        ns = NullSteer(cfg, antennas=S.A2, raw_u8=True, taps=taps)
        found = _sweep(acq, lambda i: ns.apply(_raw(i)), cfg, prns)
        assert ns.last_flags[0] == 1 and gain[0] < ns.last_gain_db[0] < gain[1], ns.last_gain_db
        ns.close()
        assert set(found) == set(want), (taps, found)
        for s, (f, d) in found.items():
            for ref in (CLEAN, want):
                dd = abs(d - ref[s][1])
                assert abs(f - ref[s][0]) <= cfg.step_freq and min(dd, cfg.code_samples - dd) <= 1, (s, f, d)
    acq.engine.close()
    assert len(S.FOUND['a', True, 5]) >= 6


N_BLOCKS = 47                   # 1.5 s of signal


def test_receiver_with_a_space_time_stage_locks_what_the_restatement_finds():
    from gpsmi.engine import Config
    from gpsmi.nulling import NullSteer
    from gpsmi.pipeline import Receiver
    cfg = Config()
    want = S.FOUND['a', True, 5]
    ns = NullSteer(cfg, antennas=S.A2, raw_u8=True, taps=5)
    rx = Receiver(cfg, raw_u8=True, antennas=S.A2, null=ns)
    assert rx.nuller is ns
    for b in range(N_BLOCKS):
        rx.feed(_raw(b))
    rx.drain()
    assert set(rx.act_sat_set) == set(want)
    locked = [rx.pool.trk.get_state(w)['phase_locked'] != 0 for w, s in enumerate(rx.pool_worker) if s]
    assert len(locked) == len(want) and all(locked)
    assert ns.last_flags[0] == 1 and ns.last_weights.shape == (1, S.A2, 5)
    rx.close()
    ns.close()                                               # (the caller's stage: the receiver left it open)


def test_run_file_null_taps_on_two_raw_recordings(tmp_path):
    """tools/run_file.py --antenna FILE --null --null-taps 5 on scene (a) written as two raw files: the
    tap count, the flag and the gain of every block in the report, the restatement's satellites
    acquired and tracked; --null-taps without --null is refused."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [str(tmp_path / f'ant{a}.bin') for a in range(S.A2)]
    files = [open(p, 'wb') for p in paths]
    for b in range(N_BLOCKS):
        for a, f in enumerate(files):
            _raw(b)[a].astype('<u2').tofile(f)
    for f in files:
        f.close()
    tool = [sys.executable, os.path.join(root, 'tools', 'run_file.py'), paths[0]]
    r = subprocess.run(tool + ['--antenna', paths[1], '--null', '--null-taps', '5', '--json'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    want = S.FOUND['a', True, 5]
    assert out['blocks'] == N_BLOCKS and out['null']['antennas'] == S.A2 and out['null']['taps'] == 5
    assert out['null']['flags'] == [1] * N_BLOCKS and all(23.5 < g < 26.0 for g in out['null']['gain_db'])
    assert {s for s, _, _ in out['acquired']} == set(want) and sorted(out['tracked']) == sorted(want)
    r = subprocess.run(tool + ['--null-taps', '5'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and '--null-taps needs --null' in r.stderr
