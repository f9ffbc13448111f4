"""The front-end stage on the GPU (gpsmi_fe_*, csrc/gpsmi_fe.hip) for the named configurations A-F
(tests/fe_ref.py): against the numpy restatement, bit-invariance to how the input is cut, no drift,
tones, and the receiver end to end on scenes rendered as other front ends record them."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import fe_ref as R
import fe_scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _engine_cfg(c):
    from gpsmi.engine import Config
    return Config() if c['fs_out'] == 2_048_000 else Config(code_samples=16368, n_cyc=8)


def _scene(c):
    from gpsmi import synth
    cfg = _engine_cfg(c)
    key = ('scene', cfg.code_samples)
    if key not in _CACHE:
        _CACHE[key] = synth.default_scene(8, seed=7, code_samples=cfg.code_samples, n_cyc=cfg.n_cyc)
    return _CACHE[key]


def _fe(c, **kw):
    from gpsmi.frontend import FrontEnd
    return FrontEnd(_engine_cfg(c), c['fs_in'], c['fmt'], c['if_hz'], passband_hz=c['passband_hz'], **kw)


def _design(c):
    from gpsmi import frontend
    return frontend.design(c['fs_in'], c['fs_out'], c['fmt'], c['if_hz'], False, c['passband_hz'])


def _input(name, seconds):
    key = ('in', name, seconds)
    if key not in _CACHE:
        c = R.CONFIGS[name]
        _CACHE[key] = S.render(_scene(c), c['fs_in'], c['fmt'], c['if_hz'], 0, int(seconds * c['fs_in']))
    return _CACHE[key]


@pytest.mark.parametrize('name', sorted(R.CONFIGS))
def test_kernel_matches_restatement(name):
    c = R.CONFIGS[name]
    x = _input(name, 0.25)
    fe = _fe(c)
    y = fe.push(x)
    K, L, T = _design(c)
    assert (fe.n_taps, fe.n_phases) == (K, L)
    P, Q = R.ratio(c['fs_in'], c['fs_out'])
    assert len(y) == R.complete(K, P, Q, len(x) // (2 if c['fmt'] in ('sc8', 'sc16') else 1))
    ref = R.run(x, c, K, L, T, n_out=len(y))
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    err = np.abs(y.astype(np.complex128) - ref).max()
    assert err <= 2e-5 * rms, (name, err / rms)
    # flush: the outputs up to the last input sample, with zeros past it
    tail = fe.flush()
    n_all = -(-(len(x) // (2 if c['fmt'] in ('sc8', 'sc16') else 1)) * Q // P)
    assert len(y) + len(tail) == n_all
    xm = R.mix(R.decode(x, c['fmt']), c['if_hz'], c['fs_in'])
    ref_t = R.resample(xm, K, L, T, P, Q, len(y), n_all)
    assert np.abs(tail - ref_t).max() <= 2e-5 * rms
    fe.close()


@pytest.mark.parametrize('name', ['A', 'B', 'D', 'E'])
def test_bits_do_not_depend_on_the_cut(name):
    from gpsmi import _lib
    from gpsmi.engine import DeviceBuffer
    import ctypes as C
    c = R.CONFIGS[name]
    x = _input(name, 0.05)
    per = 2 if c['fmt'] in ('sc8', 'sc16') else 1
    n = x.size // per
    fe = _fe(c)
    one = fe.push(x)
    fe.reset()
    rng = np.random.default_rng(5)
    cuts = [1, 7919, fe.n_taps // 3, 1, 2, fe.n_taps - 1, 0]
    while sum(cuts) < n:
        cuts.append(int(rng.integers(1, 40_000)))
    parts, pos = [], 0
    for m in cuts:
        m = min(m, n - pos)
        parts.append(fe.push(x[pos * per:(pos + m) * per]))
        pos += m
        if pos == n:
            break
    many = np.concatenate(parts)
    assert len(many) == len(one) and many.tobytes() == one.tobytes()
    # device to device, in three pieces: the same bytes
    fe.reset()
    lib = _lib.load()
    d_in, d_out = DeviceBuffer(x.nbytes), DeviceBuffer((len(one) + 16) * 8)
    d_in.upload(x)
    got, off = C.c_size_t(0), 0
    item = x.itemsize * per
    for a, b in ((0, 3), (3, n // 2), (n // 2, n)):
        _lib.check(lib.gpsmi_fe_push_dev(fe.h, d_in.at(a * item), b - a, d_out.at(off * 8), len(one) + 16 - off,
                                         C.byref(got)), 'gpsmi_fe_push_dev')
        off += got.value
    assert off == len(one)
    assert d_out.download(np.complex64, off).tobytes() == one.tobytes()
    # a call that would emit more than max_out changes nothing
    fe.reset()
    with pytest.raises(_lib.EngineError, match='max_out'):
        _lib.check(lib.gpsmi_fe_push_dev(fe.h, d_in.ptr, n, d_out.ptr, 10, C.byref(got)), 'push_dev')
    assert fe.push(x).tobytes() == one.tobytes()
    d_in.free()
    d_out.free()
    fe.close()


def test_no_drift_over_ten_seconds():
    """Config A, a complex tone in 1-s chunks: the phase of the last output is 2 pi f n / fs_out."""
    c = R.CONFIGS['A']
    f, A = 312_345.0, 0.5
    fe = _fe(c)
    fi = c['fs_in']
    outs = []
    for s in range(10):
        i = np.arange(s * fi, (s + 1) * fi, dtype=np.float64)
        x = A * np.exp(2j * np.pi * f * i / fi)
        outs.append(R.add_quantise(x, 'sc16', 1.0))
        outs[-1] = fe.push(outs[-1])
    y = np.concatenate(outs)
    n = len(y) - 1
    assert n > 10 * c['fs_out'] - 100
    want = 2 * np.pi * ((f * n) % c['fs_out']) / c['fs_out']
    d = np.angle(y[-1] * np.exp(-1j * want))
    assert abs(d) <= 1e-3, d
    assert abs(abs(y[-1]) - A) <= 0.01 * A
    fe.close()


def _components(c, kind, freq):
    """Mixed-domain frequencies of an input tone: complex at IF + freq, or a real cosine at freq (its
    two halves, each of the tone's amplitude after the stage's factor 2, at freq - IF and -freq - IF)."""
    if kind == 'complex':
        return [freq]
    return [freq - c['if_hz'], -freq - c['if_hz']]


def _tone_input(c, kind, freq, A, n, seed):
    i = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    if kind == 'complex':
        x = A * np.exp(2j * np.pi * (c['if_hz'] + freq) * i / c['fs_in'])
    else:
        x = A * np.cos(2 * np.pi * freq * i / c['fs_in'])
    lsb = 1.0 / 128.0 if c['fmt'] in ('r8', 'sc8', 'u8iq') else 1.0 / 32768.0
    x = x + lsb * rng.standard_normal(n) + (0 if kind == 'real' else 1j * lsb * rng.standard_normal(n))
    return R.add_quantise(x, c['fmt'], 1.0)


# per configuration: (kind, input frequency) of a passband tone and of a tone placed to alias or image
TONES = {
    'A': [('complex', 0.5 * 901_120.0), ('complex', 1_598_000.0)],
    'B': [('real', 4_092_000.0 + 450_000.0), ('real', 1_908_000.0)],
    'C': [('real', 9_548_000.0 - 450_000.0), ('real', 2_452_000.0)],
    'D': [('complex', -400_000.0), ('complex', 1_200_000.0)],
    'E': [('complex', 300_000.0), ('complex', 500_000.0)],
    'F': [('real', 4_092_000.0 + 1_500_000.0), ('real', 4_092_000.0 - 2_000_000.0)],
}


@pytest.mark.parametrize('name', sorted(R.CONFIGS))
def test_tones(name):
    """A passband tone comes out within 0.1 dB; whatever reaches the output band from the stopband
    (aliases of the resampling, the mirror half of real input) is >= 60 dB down."""
    c = R.CONFIGS[name]
    fi, fo, p, s = c['fs_in'], c['fs_out'], R.passband(c), R.stop_edge(c)
    A, N = 0.5, 65536
    checked = 0
    for t, (kind, freq) in enumerate(TONES[name]):
        fe = _fe(c)
        n_in = int((N + 4 * fe.n_taps) * fi / fo) + 4 * fe.n_taps
        y = fe.push(_tone_input(c, kind, freq, A, n_in, t))
        fe.close()
        y = y[2 * fe.n_taps:2 * fe.n_taps + N].astype(np.complex128)
        assert len(y) == N
        n = np.arange(N) + 2 * fe.n_taps
        w = np.hanning(N)

        def amp(f):
            return abs(np.sum(y * w * np.exp(-2j * np.pi * f * n / fo))) / w.sum()

        wanted, unwanted = [], []
        for v in _components(c, kind, freq):
            v = v - fi * np.floor(v / fi + 0.5)
            if abs(v) <= p:
                wanted.append(v)
            for k in range(-3, 4):
                u = v + k * fi
                if abs(u) < s or (k == 0 and abs(v) <= p):
                    continue
                wa = u - fo * np.floor(u / fo + 0.5)
                if abs(wa) <= 0.95 * fo / 2:
                    unwanted.append(wa)
        for v in wanted:
            assert abs(20 * np.log10(amp(v) / A)) <= 0.1, (name, kind, freq, v, amp(v))
        for u in unwanted:
            if min([abs(u - v) for v in wanted] + [1e9]) < 20_000:
                continue
            assert 20 * np.log10(amp(u) / A + 1e-30) <= -60.0, (name, kind, freq, u, amp(u))
            checked += 1
    assert checked >= 1


def _truth_delays(sc, cfg, block, prns, freqs):
    """Code phases the acquisition finds on the scene rendered directly at fs_out (the time base the
    front end must reproduce), at the bin of each SV's true Doppler."""
    from gpsmi.engine import AcqEngine
    eng = AcqEngine(cfg)
    t = eng.search(sc.block(block), prns, freqs, 4 if cfg.code_samples == 2048 else 2)
    eng.close()
    return t


@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_receiver_end_to_end(name):
    from gpsmi.pipeline import Receiver
    c = R.CONFIGS[name]
    cfg = _engine_cfg(c)
    sc = _scene(c)
    prns = [s.prn for s in sc.sats]
    x = S.render(sc, c['fs_in'], c['fmt'], c['if_hz'], 0, 3 * c['fs_in'])
    fe = _fe(c)
    blocks = [b.copy() for b in fe.blocks(x)]
    fe.close()
    assert len(blocks) == int(3.0 * 1000 // cfg.n_cyc) - 1 or len(blocks) == int(3.0 * 1000 // cfg.n_cyc)
    # acquisition: every SV within one step of its Doppler, code phase within 1 sample of the direct render
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(int((cfg.max_freq - cfg.min_freq) / cfg.step_freq))]
    from gpsmi.engine import AcqEngine
    eng = AcqEngine(cfg)
    t = eng.search(blocks[1], prns, freqs, 4)
    eng.close()
    ref = _truth_delays(sc, cfg, 1, prns, freqs)
    nm = (t['peak'].astype(np.float64) - t['mean']) / t['std']
    for col, s in enumerate(sc.sats):
        b = int(nm[:, col].argmax())
        assert nm[b, col] > cfg.corr_min, (s.prn, nm[b, col])
        assert abs(freqs[b] - s.doppler) <= cfg.step_freq, (s.prn, freqs[b], s.doppler)
        d = abs(int(t['argmax'][b, col]) - int(ref['argmax'][b, col]))
        assert min(d, cfg.code_samples - d) <= 1, (s.prn, t['argmax'][b, col], ref['argmax'][b, col])
    rx = Receiver(cfg)
    for blk in blocks:
        rx.feed(blk)
    rx.drain()
    found = {sv: (f, d) for _, sv, f, d in rx.found_sats}
    assert set(found) >= set(prns)
    for s in sc.sats:       # (the sweep takes the first bin over CORR_MIN: the best one or a neighbour)
        assert abs(found[s.prn][0] - s.doppler) <= 1.5 * cfg.step_freq, (s.prn, found[s.prn][0], s.doppler)
    assert set(rx.act_sat_set) == set(prns)
    locked = [rx.pool.trk.get_state(w)['phase_locked'] != 0 for w, s in enumerate(rx.pool_worker) if s]
    assert len(locked) == len(prns) and all(locked)
    last = pickle.loads(rx.result_list[-1])
    assert {f['SAT'] for f in last[1]} == set(prns)
    rx.close()


def test_native_16368_acquisition_and_tracking():
    """Config F (real IF at 16.368 MHz, the configs[4] path): Acquisition and TrkEngine at
    CODE_SAMPLES 16368, N_CYC 8 on the front end's output."""
    from gpsmi.engine import AcqEngine, TrkEngine
    c = R.CONFIGS['F']
    cfg = _engine_cfg(c)
    sc = _scene(c)
    x = S.render(sc, c['fs_in'], c['fmt'], c['if_hz'], 0, int(1.2 * c['fs_in']))
    fe = _fe(c)
    blocks = [b.copy() for b in fe.blocks(x)]
    fe.close()
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    eng = AcqEngine(cfg)
    t = eng.search(blocks[1], prns, freqs, 2)
    eng.close()
    ref = _truth_delays(sc, cfg, 1, prns, freqs)
    nm = (t['peak'].astype(np.float64) - t['mean']) / t['std']
    trk = TrkEngine(cfg, max_ch=len(prns))
    for col, s in enumerate(sc.sats):
        b = int(nm[:, col].argmax())
        assert nm[b, col] > cfg.corr_min, (s.prn, nm[b, col])
        assert abs(freqs[b] - s.doppler) <= cfg.step_freq
        d = abs(int(t['argmax'][b, col]) - int(ref['argmax'][b, col]))
        assert min(d, cfg.code_samples - d) <= 1, (s.prn, t['argmax'][b, col], ref['argmax'][b, col])
        trk.open(col, s.prn, freqs[b], int(t['argmax'][b, col]))
    for blk in blocks[2:]:
        trk.process(blk)
    for col, s in enumerate(sc.sats):
        assert trk.get_state(col)['phase_locked'] != 0, s.prn
    trk.close()


def test_run_file_position_fix_from_sc16_at_4_msps(tmp_path):
    """tools/run_file.py --format sc16 --fs 4000000 on a 22-s geometric scene rendered at 4 Msps: a
    fix within 5 m of the truth (the bar of test_recording_to_position_fix)."""
    from gpsmi import position as P, synth_nav
    seconds = 22.0
    truth = np.array(P.geo_to_ecef(49.082961, 8.307581, 160.0))
    sc, info = synth_nav.geometric_scene(truth, seconds)
    path = str(tmp_path / 'usrp_sc16.bin')
    S.write(path, sc, 4_000_000, 'sc16', 0.0, seconds)
    eph = str(tmp_path / 'gpsEphem.json')
    with open(eph, 'w') as f:
        json.dump({str(k): v for k, v in info['ephs'].items()}, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path, '--ephemeris', eph,
                        '--format', 'sc16', '--fs', '4000000', '--json'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['blocks'] >= int(seconds / 0.032) - 1 and len(out['tracked']) >= 6
    assert out['fixes'] > 150
    pos = np.array(out['position']['ecef_m'])
    assert np.linalg.norm(pos - truth) < 5.0, np.linalg.norm(pos - truth)
