"""Narrowband interference excision on the GPU (gpsmi_ifx_*, csrc/gpsmi_ifx.hip) against the numpy
restatement (tests/ifx_ref.py), and what it buys: acquisition and tracking through a CW jammer."""
import pickle

import numpy as np
import pytest

import ifx_ref as R

pytestmark = pytest.mark.gpu

JN_DB, TONE_HZ = 35.0, -2717.3
FACTOR = 4
_CACHE = {}


def _scene():
    from gpsmi import synth
    if 'scene' not in _CACHE:
        _CACHE['scene'] = synth.default_scene(8, seed=7)
    return _CACHE['scene']


def _blocks(first, count, jn_db=JN_DB):
    """complex64 blocks of the scene before quantisation, with the CW tone (jn_db None: clean)."""
    sc = _scene()
    out = []
    for b in range(first, first + count):
        key = (b, jn_db)
        if key not in _CACHE:
            x = sc.block_float(b)
            if jn_db is not None:
                x = R.add_tone(x, jn_db, TONE_HZ, sc.sample_rate, b * sc.ngps, sc.noise_sigma ** 2)
            _CACHE[key] = x.astype(np.complex64)
        out.append(_CACHE[key])
    return out


def _rms(x):
    return float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)))


def test_kernel_matches_restatement():
    from gpsmi.excision import Excision
    xs = _blocks(0, 4)
    ex = Excision()
    ref = R.ExcisionRef(_scene().ngps)
    orc = R.Oracle32(_scene().ngps)              # float32 of the same arithmetic: what the format costs
    borderline = []
    for b, x in enumerate(xs):
        y = ex.apply(x)
        gm = R.words_to_mask(ex.last_masks[0])
        carry = ref.carry.copy()
        y_ref, count, mask, P, thr = ref.process(x)
        diff = np.flatnonzero(gm != mask)
        for k in diff:          # (a bin this close to the threshold may fall either way in float32)
            assert abs(P[k] - thr) <= 1e-4 * thr, (b, k, P[k], thr)
            borderline.append((b, int(k)))
        if len(diff):
            nxt = ref.carry
            ref.carry = carry
            y_ref = ref.excise_with(x, gm)
            ref.carry = nxt
        assert ex.last_counts[0] == (count if not len(diff) else gm.sum())
        assert 0 < ex.last_counts[0] <= 256
        # FACTOR x the float32 oracle's own distance from float64 (tests/test_gpu_excision_ref.py),
        # and never more than the 1e-4 this test used to allow
        dev = float(np.abs(orc.overlap_add(orc.spectra(x), gm) - y_ref).max()) / _rms(x)
        orc.carry = x[-R.H:].copy()
        err = float(np.abs(y - y_ref).max()) / _rms(x)
        print(f'block {b}: output error {err:.3e}, bound {FACTOR * dev:.3e}')
        assert 0 < dev and err <= min(1e-4, FACTOR * dev), (b, err, FACTOR * dev)
    if borderline:
        print(f'bins within 1e-4 of the threshold that differ (allowed): {borderline}')
    ex.close()

    off = Excision(thresh_db=float('inf'))
    for x in xs:
        y = off.apply(x)
        assert off.last_counts[0] == 0 and not off.last_masks.any()
        assert np.abs(y - x).max() <= 1e-5 * _rms(x)
    off.close()


def test_batched_call_equals_single_calls_and_reset():
    from gpsmi.engine import DeviceBuffer
    from gpsmi.excision import Excision
    xs = np.stack(_blocks(0, 4))
    n = xs.shape[1]
    d_in, d_out = DeviceBuffer(xs.nbytes), DeviceBuffer(xs.nbytes)
    d_in.upload(xs)
    ex = Excision()
    ex.apply_dev(d_in.ptr, d_out.ptr, 4)
    batched = d_out.download(np.complex64, 4 * n)
    counts, masks = ex.last_counts.copy(), ex.last_masks.copy()
    ex.reset()
    for b in range(4):
        ex.apply_dev(d_in.at(b * n * 8), d_out.at(b * n * 8), 1)
        assert ex.last_counts[0] == counts[b] and np.array_equal(ex.last_masks[0], masks[b])
    single = d_out.download(np.complex64, 4 * n)
    assert batched.tobytes() == single.tobytes()
    ex.reset()
    ex.apply_dev(d_in.ptr, d_out.ptr, 1)
    assert d_out.download(np.complex64, n).tobytes() == batched[:n].tobytes()
    # the host entry point gives the same bytes; in-place is refused
    ex.reset()
    assert ex.apply(xs).tobytes() == batched.tobytes()
    from gpsmi._lib import EngineError
    with pytest.raises(EngineError, match='overlap'):
        ex.apply_dev(d_in.ptr, d_in.ptr, 1)
    ex.close()
    d_in.free()
    d_out.free()


def test_u8_input_equals_complex64_of_the_decode():
    from gpsmi import synth
    from gpsmi.excision import Excision
    sc = _scene()
    raw = np.stack([R.quantise(R.add_tone(sc.block_float(b), 0.0, TONE_HZ, sc.sample_rate, b * sc.ngps,
                                          sc.noise_sigma ** 2)) for b in range(3)])
    ex_u8, ex_c = Excision(raw_u8=True), Excision()
    y_u8 = ex_u8.apply(raw)
    y_c = ex_c.apply(synth.raw_to_c64(raw))
    assert (ex_u8.last_counts > 0).all()
    assert np.array_equal(ex_u8.last_counts, ex_c.last_counts)
    assert np.array_equal(ex_u8.last_masks, ex_c.last_masks)
    assert y_u8.tobytes() == y_c.tobytes()
    ex_u8.close()
    ex_c.close()


def test_acquisition_through_the_jammer():
    """Fails without excision: the tone buries every SV below CORR_MIN."""
    from gpsmi.engine import AcqEngine, Config
    from gpsmi.excision import Excision
    cfg = Config()
    sc = _scene()
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    clean = _blocks(1, 1, None)[0]
    jam = _blocks(0, 2)
    ex = Excision()
    cleaned = ex.apply(np.stack(jam))[1]
    ex.close()
    eng = AcqEngine(cfg)

    def table(x):            # normMaxCorr (gpsrecv.py:223) and argmax of every (bin, SV) cell
        t = eng.search(x, prns, freqs, 4)
        return (t['peak'].astype(np.float64) - t['mean']) / t['std'], t['argmax']

    nm_c, am_c = table(clean)
    nm_j, _ = table(jam[1])
    nm_x, am_x = table(cleaned)
    eng.close()
    col = np.arange(len(prns))
    best_c = nm_c.argmax(axis=0)
    assert (nm_c.max(axis=0) > cfg.corr_min).all()
    assert (nm_j.max(axis=0) > cfg.corr_min).sum() <= 1, nm_j.max(axis=0)
    assert (nm_x.max(axis=0) > cfg.corr_min).all(), nm_x.max(axis=0)
    assert np.array_equal(nm_x.argmax(axis=0), best_c)
    d = np.abs(am_x[best_c, col].astype(np.int64) - am_c[best_c, col])
    assert (np.minimum(d, cfg.code_samples - d) <= 1).all()


def test_receiver_with_excision_equals_receiver_on_excised_blocks():
    from gpsmi.excision import Excision
    from gpsmi.pipeline import Receiver
    xs = _blocks(0, 64)
    ex = Excision()
    cleaned = ex.apply(np.stack(xs))
    ex.close()
    rx_a, rx_b = Receiver(excise=True), Receiver()
    for x, y in zip(xs, cleaned):
        ra, rb = rx_a.feed(x), rx_b.feed(np.ascontiguousarray(y))
        assert ra == rb
    rx_a.drain()
    rx_b.drain()
    assert rx_a.result_list == rx_b.result_list and len(rx_a.result_list) >= 1
    prns = {s.prn for s in _scene().sats}
    assert set(rx_a.act_sat_set) == prns
    locked = [rx_a.pool.trk.get_state(w)['phase_locked'] != 0
              for w, s in enumerate(rx_a.pool_worker) if s]
    assert len(locked) == len(prns) and all(locked)
    last = pickle.loads(rx_a.result_list[-1])
    assert {f['SAT'] for f in last[1]} == prns
    rx_a.close()
    rx_b.close()


def test_unsupported_config_and_wideband_pass_through():
    from gpsmi.engine import Config, EngineError
    from gpsmi.excision import Excision
    with pytest.raises(EngineError, match=r'\(-5\)'):
        Excision(Config(code_samples=16368, n_cyc=8))
    sc = _scene()
    x = sc.block_float(1)
    spec = np.zeros(sc.ngps, dtype=np.complex128)
    spec[4000:20000] = np.exp(2j * np.pi * np.random.default_rng(3).random(16000))
    x = (x + np.fft.ifft(spec) * np.sqrt(sc.ngps) * 3.0).astype(np.complex64)
    ex = Excision()
    y = ex.apply(x)
    assert ex.last_counts[0] == -1 and not ex.last_masks.any()
    assert y.tobytes() == x.tobytes()
    ex.close()


def test_run_file_excise_on_a_raw_recording(tmp_path):
    """tools/run_file.py --excise: raw uint16 in, the excision decodes, the engines run on its output."""
    import json
    import os
    import subprocess
    import sys
    sc = _scene()
    path = str(tmp_path / 'jammed.bin')
    with open(path, 'wb') as f:
        for b in range(40):
            x = R.add_tone(sc.block_float(b), 0.0, TONE_HZ, sc.sample_rate, b * sc.ngps, sc.noise_sigma ** 2)
            R.quantise(x).astype('<u2').tofile(f)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'run_file.py'), path, '--excise', '--json'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['blocks'] == 40 and out['datagrams'] >= 1
    assert {s for s, _, _ in out['acquired']} == {s.prn for s in sc.sats}
    assert sorted(out['tracked']) == sorted(s.prn for s in sc.sats)
