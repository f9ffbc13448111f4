"""Pulse blanking on the GPU (gpsmi_pb_*, csrc/gpsmi_pb.hip) against the numpy restatement
(tests/pb_ref.py), bit for bit, and what it buys: acquisition and tracking through pulsed and chirp
jammers, at 2.048 and 16.368 Msps."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ifx_ref
import pb_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PULSE_DB, CHIRP_DB, TONE_DB, TONE_HZ = 30.0, 35.0, 35.0, -2717.3
TONE_PULSE_DB = 20.0            # (pulses beside the tone: see test_receiver_excise_then_blank_on_tone_and_pulses)
_CACHE = {}


def _scene(code_samples=2048, n_cyc=32):
    from gpsmi import synth
    key = ('scene', code_samples)
    if key not in _CACHE:
        _CACHE[key] = synth.default_scene(8, seed=7, code_samples=code_samples, n_cyc=n_cyc)
    return _CACHE[key]


def _pulsed(b, sc=None, tone=False, clean=False):
    """complex128 block b of the scene with pulses (and a CW tone); clean: neither."""
    sc = sc or _scene()
    key = ('pulsed', sc.code_samples, b, tone, clean)
    if key not in _CACHE:
        x = sc.block_float(b)
        if not clean:
            # (8-sample bursts at 2.048 Msps, as long in time at any rate)
            width = 8 * sc.code_samples // 2048
            x = R.add_pulses(x, sc.noise_sigma ** 2, seed=1000 + b, jn_db=TONE_PULSE_DB if tone else PULSE_DB,
                             width=width)[0]
        if tone:
            x = ifx_ref.add_tone(x, TONE_DB, TONE_HZ, sc.sample_rate, b * sc.ngps, sc.noise_sigma ** 2)
        _CACHE[key] = x
    return _CACHE[key]


def _c64(blocks):
    return np.stack([np.asarray(x, dtype=np.complex64) for x in blocks])


def _chirped(b):
    sc = _scene()
    return sc.block_float(b) + R.chirp(b * sc.ngps, sc.ngps, sc.sample_rate, CHIRP_DB, sc.noise_sigma ** 2)


def _same(blk, ref, xs, y):
    """The GPU call's output and per-block results equal the restatement's bit for bit."""
    y_r, c_r, f_r, m_r = ref.run(xs)
    assert np.array_equal(blk.last_counts, c_r), (blk.last_counts, c_r)
    assert blk.last_floors.tobytes() == f_r.tobytes(), (blk.last_floors, f_r)
    assert blk.last_masks.tobytes() == m_r.tobytes()
    assert np.asarray(y).reshape(y_r.shape).tobytes() == y_r.tobytes()
    return c_r


def test_kernel_matches_restatement_bitwise():
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import Config
    sc = _scene()
    n = sc.ngps
    xs = _c64([_pulsed(b) for b in range(4)])
    pb = PulseBlanker()
    c = _same(pb, R.BlankerRef(n), xs, pb.apply(xs))
    assert (c > 0).all() and (c < n // 2).all()
    pb.close()

    sc16 = _scene(16368, 8)
    cfg16 = Config(code_samples=16368, n_cyc=8)
    xs16 = _c64([_pulsed(b, sc16) for b in range(3)])
    pb16 = PulseBlanker(cfg16)
    assert pb16.pre == pb16.post == 16
    c = _same(pb16, R.BlankerRef(sc16.ngps, pre=16, post=16), xs16, pb16.apply(xs16))
    assert (c > 0).all()
    pb16.close()

    # edges: all zero, constant power, a spike at the last sample (carry), over 50 % blanked, then +inf
    spike = np.asarray(_pulsed(5, clean=True), dtype=np.complex64).copy()
    spike[n - 1] = 40.0
    heavy = R.add_pulses(_pulsed(6, clean=True), sc.noise_sigma ** 2, seed=3, duty=0.4)[0]   # (+ guards: > 50 %)
    edges = _c64([np.zeros(n), np.full(n, 0.25 - 0.5j), spike, _pulsed(7, clean=True), heavy, _pulsed(1)])
    pb = PulseBlanker(pre=3, post=5)
    c = _same(pb, R.BlankerRef(n, pre=3, post=5), edges, pb.apply(edges))
    assert c[0] == 0 and c[1] == 0 and c[4] == -1
    assert pb.last_masks[3][0] & 0b11111 == 0b11111            # (the spike's carry)
    pb.close()
    off = PulseBlanker(thresh_db=float('inf'))
    y = off.apply(edges)
    assert (off.last_counts == 0).all() and not off.last_masks.any() and y.tobytes() == edges.tobytes()
    _same(off, R.BlankerRef(n, thresh_db=np.inf), edges, y)
    off.close()


def test_u8_input_equals_complex64_of_the_decode():
    from gpsmi import synth
    from gpsmi.blanking import PulseBlanker
    raw = np.stack([ifx_ref.quantise(_pulsed(b)) for b in range(3)])
    pb_u8, pb_c = PulseBlanker(raw_u8=True), PulseBlanker()
    y_u8 = pb_u8.apply(raw)
    y_c = pb_c.apply(synth.raw_to_c64(raw))
    assert (pb_u8.last_counts > 0).all()
    for k in ('last_counts', 'last_floors', 'last_masks'):
        assert getattr(pb_u8, k).tobytes() == getattr(pb_c, k).tobytes(), k
    assert y_u8.tobytes() == y_c.tobytes()
    pb_u8.close()
    pb_c.close()


def test_batching_chunking_and_reset_do_not_change_the_bits():
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import DeviceBuffer
    xs = _c64([_pulsed(b) for b in range(4)])
    n = xs.shape[1]
    d_in, d_out = DeviceBuffer(xs.nbytes), DeviceBuffer(xs.nbytes)
    d_in.upload(xs)
    pb = PulseBlanker()
    pb.apply_dev(d_in.ptr, d_out.ptr, 4)
    batched = d_out.download(np.complex64, 4 * n)
    res = [pb.last_counts.copy(), pb.last_floors.copy(), pb.last_masks.copy()]
    for cut in ([1, 3], [1, 1, 1, 1]):
        pb.reset()
        b0 = 0
        for k in cut:
            pb.apply_dev(d_in.at(b0 * n * 8), d_out.at(b0 * n * 8), k)
            assert np.array_equal(pb.last_counts, res[0][b0:b0 + k])
            assert pb.last_floors.tobytes() == res[1][b0:b0 + k].tobytes()
            assert np.array_equal(pb.last_masks, res[2][b0:b0 + k])
            b0 += k
        assert d_out.download(np.complex64, 4 * n).tobytes() == batched.tobytes()
    pb.reset()
    assert pb.apply(xs).tobytes() == batched.tobytes()           # apply == apply_dev
    pb.reset()
    pb.apply_dev(d_in.ptr, d_out.ptr, 1)                         # reset restores the first result
    assert d_out.download(np.complex64, n).tobytes() == batched[:n].tobytes()
    from gpsmi._lib import EngineError
    with pytest.raises(EngineError, match='overlap'):
        pb.apply_dev(d_in.ptr, d_in.ptr, 1)
    pb.close()
    d_in.free()
    d_out.free()

    # a call of 20 blocks (the large-call slices) over chunks of 1 MiB (2 blocks) equals 20 single calls
    xs20 = _c64([_pulsed(b % 4) for b in range(20)])
    os.environ['GPSMI_PB_CHUNK_MIB'] = '1'
    try:
        pb_chunked = PulseBlanker()
    finally:
        del os.environ['GPSMI_PB_CHUNK_MIB']
    pb1 = PulseBlanker()
    y20 = pb_chunked.apply(xs20)
    counts20 = pb_chunked.last_counts.copy()
    singles = np.stack([pb1.apply(x) for x in xs20])
    assert y20.tobytes() == singles.tobytes()
    _same(pb_chunked, R.BlankerRef(n), xs20, y20)
    assert (counts20 > 0).all()
    pb_chunked.close()
    pb1.close()


def _nm_table(eng, x, prns, freqs):
    t = eng.search(x, prns, freqs, 4)
    return (t['peak'].astype(np.float64) - t['mean']) / t['std'], t['argmax']


@pytest.mark.parametrize('jammer', ['pulsed', 'chirp'])
def test_acquisition_through_the_jammers(jammer):
    """Fails without blanking: the jammer buries the satellites below CORR_MIN."""
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import AcqEngine, Config
    cfg = Config()
    sc = _scene()
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    jam = _c64([_pulsed(b) for b in (0, 1)] if jammer == 'pulsed' else [_chirped(b) for b in (0, 1)])
    clean = np.asarray(sc.block_float(1), dtype=np.complex64)
    pb = PulseBlanker()
    blanked = pb.apply(jam)[1]
    assert 0 < pb.last_counts[1] < sc.ngps // 2
    pb.close()
    eng = AcqEngine(cfg)
    nm_c, am_c = _nm_table(eng, clean, prns, freqs)
    nm_j, _ = _nm_table(eng, jam[1], prns, freqs)
    nm_x, am_x = _nm_table(eng, blanked, prns, freqs)
    eng.close()
    col = np.arange(len(prns))
    best_c = nm_c.argmax(axis=0)
    assert (nm_c.max(axis=0) > cfg.corr_min).all()
    assert (nm_j.max(axis=0) > cfg.corr_min).sum() <= 1, nm_j.max(axis=0)
    assert (nm_x.max(axis=0) > cfg.corr_min).all(), nm_x.max(axis=0)
    # the clean run's bin, or its neighbour for an SV between two bins (zeroing a third of the samples
    # in a 50-kHz pattern, the chirp, tips the balance of two near-equal bins), and its code phase there
    best_x = nm_x.argmax(axis=0)
    assert (np.abs(best_x - best_c) <= (0 if jammer == 'pulsed' else 1)).all(), (best_x, best_c)
    d = np.abs(am_x[best_x, col].astype(np.int64) - am_c[best_x, col])
    assert (np.minimum(d, cfg.code_samples - d) <= 1).all()


def test_acquisition_at_16368_through_pulses():
    """The excision refuses CODE_SAMPLES 16368; the blanking runs there."""
    from gpsmi.acquisition import Acquisition
    from gpsmi.blanking import PulseBlanker
    from gpsmi.engine import Config
    cfg = Config(code_samples=16368, n_cyc=8)
    sc = _scene(16368, 8)
    xs = _c64([_pulsed(b, sc) for b in (0, 1)])
    pb = PulseBlanker(cfg)
    blanked = pb.apply(xs)[1]
    assert pb.last_counts[1] > 0
    pb.close()
    prns = [s.prn for s in sc.sats]
    freqs = [cfg.min_freq + cfg.step_freq * i for i in range(50)]
    acq = Acquisition(cfg)
    t = acq.search_table(blanked, prns, freqs, 4)
    acq.engine.close()
    nm = (t['peak'].astype(np.float64) - t['mean']) / t['std']
    for col, s in enumerate(sc.sats):
        b = int(nm[:, col].argmax())
        assert nm[b, col] > cfg.corr_min, (s.prn, nm[b, col])
        assert abs(freqs[b] - s.doppler) <= cfg.step_freq, (s.prn, freqs[b], s.doppler)


def _locked(rx):
    return [rx.pool.trk.get_state(w)['phase_locked'] != 0 for w, s in enumerate(rx.pool_worker) if s]


def _run_pair(rx_a, rx_b, xs_a, xs_b):
    for a, b in zip(xs_a, xs_b):
        assert rx_a.feed(a) == rx_b.feed(np.ascontiguousarray(b))
    rx_a.drain()
    rx_b.drain()
    assert rx_a.result_list == rx_b.result_list and len(rx_a.result_list) >= 1
    prns = {s.prn for s in _scene().sats}
    assert set(rx_a.act_sat_set) == prns
    locked = _locked(rx_a)
    assert len(locked) == len(prns) and all(locked)
    assert {f['SAT'] for f in pickle.loads(rx_a.result_list[-1])[1]} == prns
    rx_a.close()
    rx_b.close()


def test_receiver_with_blanking_equals_receiver_on_blanked_blocks():
    from gpsmi.blanking import PulseBlanker
    from gpsmi.pipeline import Receiver
    xs = _c64([_pulsed(b) for b in range(64)])
    pb = PulseBlanker()
    blanked = pb.apply(xs)
    pb.close()
    _run_pair(Receiver(blank=True), Receiver(), xs, blanked)


def test_receiver_excise_then_blank_on_tone_and_pulses():
    """A tone 35 dB up and pulses 20 dB up.  (Pulses 30 dB up raise the excision's median spectrum
    150-fold, which hides the tone's Hann sidelobes from it: what is left of them costs the weakest SV.)"""
    from gpsmi.blanking import PulseBlanker
    from gpsmi.excision import Excision
    from gpsmi.pipeline import Receiver
    xs = _c64([_pulsed(b, tone=True) for b in range(64)])
    ex, pb = Excision(), PulseBlanker()
    cleaned = pb.apply(ex.apply(xs))
    ex.close()
    pb.close()
    _run_pair(Receiver(blank=True, excise=True), Receiver(), xs, cleaned)


def test_receiver_raw_u8_with_blanking():
    from gpsmi.blanking import PulseBlanker
    from gpsmi.pipeline import Receiver
    raw = np.stack([ifx_ref.quantise(_pulsed(b)) for b in range(64)])
    pb = PulseBlanker(raw_u8=True)
    blanked = pb.apply(raw)
    pb.close()
    _run_pair(Receiver(raw_u8=True, blank=True), Receiver(), raw, blanked)
    with pytest.raises(ValueError, match='PulseBlanker'):
        Receiver(raw_u8=True, blank=PulseBlanker())


def test_receiver_with_blanking_on_a_clean_scene_acquires_the_same():
    from gpsmi.pipeline import Receiver
    sc = _scene()
    rx_a, rx_b = Receiver(blank=True), Receiver()
    for b in range(64):
        x = sc.block(b)
        rx_a.feed(x)
        rx_b.feed(x)
        if not rx_a.sweep_all_freq and not rx_b.sweep_all_freq:
            break
    found_a = {sv: (f, d) for _, sv, f, d in rx_a.found_sats}
    found_b = {sv: (f, d) for _, sv, f, d in rx_b.found_sats}
    assert set(found_a) == set(found_b) == {s.prn for s in sc.sats}
    # (the sweep takes the first bin over CORR_MIN: for an SV between two bins, the few noise samples
    # blanked in a clean block may decide which of the two comes first)
    for sv, (f, d) in found_b.items():
        assert abs(found_a[sv][0] - f) <= rx_b.cfg.step_freq, (sv, found_a[sv], (f, d))
        if found_a[sv][0] == f:                  # (the code phase: the same within a sample)
            dd = abs(int(found_a[sv][1]) - int(d))
            assert min(dd, sc.code_samples - dd) <= 1, (sv, found_a[sv], (f, d))
    rx_a.close()
    rx_b.close()


def test_run_file_blank_on_a_raw_recording(tmp_path):
    """tools/run_file.py --blank: raw uint16 in, the blanker decodes, the engines run on its output."""
    sc = _scene()
    path = str(tmp_path / 'pulsed.bin')
    with open(path, 'wb') as f:
        for b in range(40):
            ifx_ref.quantise(_pulsed(b)).astype('<u2').tofile(f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_file.py'), path, '--blank', '--json'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['blocks'] == 40 and out['datagrams'] >= 1
    assert {s for s, _, _ in out['acquired']} == {s.prn for s in sc.sats}
    assert sorted(out['tracked']) == sorted(s.prn for s in sc.sats)
